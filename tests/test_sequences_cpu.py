"""The sequence harness of tests/seq_model.py without a GPU: the generator is deterministic, the committed seeds cover what they have to
cover, few ops are inert, and the model tells every deliberate bookkeeping slip (seq_model.MUTANTS) from the truth.  For the many-map
device calls (seq_model.NEW_KINDS): the committed seeds keep every op they had before those were inserted, every call occurs in every
shape, follows and precedes a writer of its map on another stream with no host synchronisation between them, one run of them is longer
than the ring they share, and every cloud call occurs chained to a batch (also on another stream than the batch) and foreign.
For the six calls on caller-held planes (seq_model.PLANE_KINDS, tests/seq_planes.py): the lists from before them are kept, every chain the
header names occurs, every kind reads what an op on another stream wrote since the last checkpoint, a chain's buffer is overwritten
while a call on another stream may still read it, one run per sequence holds all six on two caller streams and goes round the ring,
shifts are sums of several moves, end with a reset and reach a side, the rows of a call are used to the last, and few calls are inert.
For gg_box_clusters, gg_score_rollouts and gg_clearance_clouds in plane mode (seq_model.LATE_KINDS, tests/seq_late.py): the lists from
before them are kept, every chain occurs, every kind reads what an op on another stream wrote since the last checkpoint, a box call
follows and precedes a move of its map on another stream (one stands between it and the cluster call it reads), one run per sequence
holds more rollout calls with different starts than the ring has entries, a distance buffer is overwritten that a rollout call on
another stream read, the rows of a call are used to the last, the sizes stay small, and few calls are inert.

`python -m tests.test_sequences_cpu` prints the coverage table and the mutant table of DESIGN.md.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import seq_model as sm  # noqa: E402
from tests import seq_late as sl  # noqa: E402
from tests import seq_planes as sp  # noqa: E402

# the committed seeds: tests/test_sequences_gpu.py runs exactly these
SEEDS = {"latency": [0, 1], "fleet": [0, 1], "server": [0, 1]}
CASES = [(shape, seed) for shape in ("fleet", "latency", "server") for seed in SEEDS[shape]]   # (cheapest model first)


@functools.lru_cache(maxsize=None)
def sequence(shape, seed):
    return sm.make_sequence(seed, shape)


@functools.lru_cache(maxsize=None)
def truth(shape, seed):
    """(results per op, state per slot, [(op index, points inside the map)] per filtered cloud, the planes and notes the model keeps per op)
    of the true model"""
    model = sm.ContextModel(shape).bind(sequence(shape, seed))
    inside = []
    results = []
    for i, op in enumerate(sequence(shape, seed)):
        results.append(model.apply(op, i))
        for s in (sm.touched(op, model.n) if op["op"] in sm.FILTERS else []):
            inside.append((i, int((model.slots[s].last[0] != sm.oracle.OUTSIDE).sum())))
    return results, [model.state(s) for s in range(model.n)], inside, model.outs


def differs(a, b):
    if (a is None) != (b is None):
        return "one of the two returns nothing"
    return sm.first_diff(a, b) or sm.first_diff(b, a)


def distinguishes(shape, seed, mutant=None, drop=None):
    """None, or where a wrong model (`mutant`) / the sequence without its ops of kind `drop` first differs from the truth in something the
    driver compares: an op's results, or a slot's final state"""
    results, states = truth(shape, seed)[:2]
    model = sm.ContextModel(shape, mutant=mutant).bind(sequence(shape, seed))
    for i, op in enumerate(sequence(shape, seed)):
        if op["op"] == drop:
            continue
        if drop == "filter_batch" and op.get("source", {}).get("mode") == "chained":
            continue   # (a cloud call on the buffers of a batch that is gone: nothing to say about it)
        d = differs(results[i], model.apply(op, i))
        if d:
            return f"op {i} ({op['op']}): {d}"
    for s in range(model.n):
        d = differs(states[s], model.state(s))
        if d:
            return f"final state of slot {s}: {d}"
    return None


def first_kill(**what):
    for shape, seed in CASES:
        d = distinguishes(shape, seed, **what)
        if d:
            return shape, seed, d
    return None


# ---------------------------------------------------------------------------------------------------------------- determinism

def test_the_same_seed_gives_the_same_json():
    for shape, seed in CASES:
        a, b = json.dumps(sm.make_sequence(seed, shape)), json.dumps(sm.make_sequence(seed, shape))
        assert a == b and json.loads(a) == sequence(shape, seed)
    assert json.dumps(sm.make_sequence(0, "fleet")) != json.dumps(sm.make_sequence(1, "fleet"))
    assert sm.make_sequence(7, "latency")[-1] == {"op": "checkpoint"}   # (any seed gives a sequence, not only the committed ones)


def test_launch_tunings_are_fixed_at_the_start_and_no_fault_injection():
    for shape, seed in CASES:
        ops = sequence(shape, seed)
        assert ops[0]["op"] == "tunings" and all(op["op"] != "tunings" for op in ops[1:])
        assert set(ops[0]) == {"op", "graphs", "halves_min_clouds", "front", "sweep_waves", "scan_parts", "move_chunk", "export_variant"}
    assert {sequence("latency", s)[0]["graphs"] for s in SEEDS["latency"]} == {0, 1}   # graphs on in half of the latency seeds


# ---------------------------------------------------------------------------------------------------------------- coverage

def coverage_table():
    """{predicate or "any": {kind: how many ops of that kind met a slot for which the predicate held}} over the committed seeds"""
    table = {p: {k: 0 for k in sm.KINDS if sm.allowed(p, k)} for p in sm.PREDICATES}
    table["any"] = {k: 0 for k in sm.KINDS}
    for shape, seed in CASES:
        pred = sm.Predicates(sm.SHAPES[shape]["n_slots"])
        for op in sequence(shape, seed):
            k = op["op"]
            if k in table["any"]:
                table["any"][k] += 1
                slots = sm.touched(op, pred.n)
                for p in sm.PREDICATES:
                    if k in table[p] and pred.holds(p, slots):
                        table[p][k] += 1
            pred.apply(op)
    return table


def test_every_op_kind_occurs():
    missing = [k for k, c in coverage_table()["any"].items() if c == 0]
    assert not missing, missing


def size_class(count):
    return next(name for name, (lo, hi) in sm.CLASS_RANGE.items() if lo <= count <= hi)


def test_every_batch_size_class_and_stream_choice_occurs_in_every_shape_that_can_take_it():
    for shape in sm.SHAPES:
        ops = [op for seed in SEEDS[shape] for op in sequence(shape, seed)]
        classes = {size_class(len(op["slots"])) for op in ops if op["op"] == "filter_batch"}
        assert classes == set(sm.SHAPES[shape]["classes"]), (shape, classes)
        for kind, names in (("filter_batch", sm.MAP_STREAMS), ("export_layers", sm.MAP_STREAMS), ("reset_maps", sm.MAP_STREAMS), ("move_maps", sm.MAP_STREAMS)):
            seen = {op["stream"] for op in ops if op["op"] == kind}
            assert seen == set(names), (shape, kind, seen)
        pads = {bool(op["pad"]) for op in ops if op["op"] == "export_layers"}
        assert pads == {False, True}, (shape, "an export with planes further apart than they are long, and one without")
        fmts = {(op["fmt"], op["tfs"] is not None) for op in ops if op["op"] == "filter_batch"}
        assert fmts == {(16, False), (16, True), (32, False), (32, True)}, (shape, fmts)
    outputs = {tuple(op["outputs"]) for shape, seed in CASES for op in sequence(shape, seed) if op["op"] == "filter_batch"}
    for name in ("labels", "out_index", "counts", "masks", "pc2", "out_clouds"):
        assert any(name in o for o in outputs) and any(name not in o for o in outputs), name


def test_every_predicate_meets_every_op_kind_the_header_allows():
    table = coverage_table()
    empty = [(p, k) for p in sm.PREDICATES for k, c in table[p].items() if c == 0]
    assert not empty, empty


def test_every_gpu_sequence_has_device_ops_in_a_row_on_two_streams():
    for shape, seed in CASES:
        best, run, streams = 0, 0, set()
        for op in sequence(shape, seed):
            if op["op"] in sm.DEVICE_KINDS:
                run += 1
                streams.add(op.get("stream"))
                if len(streams) >= 2:
                    best = max(best, run)
            else:
                run, streams = 0, set()
        assert best >= 3, (shape, seed, best)


# ---------------------------------------------------------------------------------------------------------------- the many-map device calls

# length and sha256 (first 32 hex digits, of json.dumps(ops, sort_keys=True)) of every committed list as it was before the ops of
# sm.NEW_KINDS were inserted
BEFORE_THE_DEVICE_CALLS = {
    ("latency", 0): (132, "969a6780750e76b3576de63fdf7a51c3"),
    ("latency", 1): (134, "fb94a7f1493e139c4348704e93e630ae"),
    ("fleet", 0): (272, "d6ca014acda7a922a93bd2de08f91c41"),
    ("fleet", 1): (261, "6cac62b3a85789751fb477ec3701776a"),
    ("server", 0): (131, "b9ea3904a2ffdd3e4c33be63d35b75c9"),
    ("server", 1): (132, "72074d3428f0b1a7e553aa8666d13c11"),
}


def test_the_committed_seeds_keep_every_op_they_had():
    """make_sequence(.., device_calls=False) is the list from before the device calls were added, dict for dict, and a subsequence of the
    full list: the same dicts in the same order"""
    for shape, seed in CASES:
        old = sm.make_sequence(seed, shape, device_calls=False)
        assert (len(old), hashlib.sha256(json.dumps(old, sort_keys=True).encode()).hexdigest()[:32]) == BEFORE_THE_DEVICE_CALLS[(shape, seed)], (shape, seed)
        assert not any(op["op"] in sm.NEW_KINDS for op in old)
        rest = iter(sequence(shape, seed))
        for i, op in enumerate(old):
            assert any(op == other for other in rest), (shape, seed, i, "is missing from the full list, or out of order")


def test_every_device_call_occurs_in_every_shape():
    for shape in sm.SHAPES:
        seen = {op["op"] for seed in SEEDS[shape] for op in sequence(shape, seed)}
        assert set(sm.NEW_KINDS) <= seen, (shape, set(sm.NEW_KINDS) - seen)


def ordered_pairs(ops):
    """{(kind of the earlier op, kind of the later op)} over the pairs of device ops that name a common map, run on two different streams
    and have no host-synchronising op between them (in the style of consecutive_device_ops of tests/test_sequences_gpu.py)"""
    pairs, run = set(), []
    for op in ops:
        if op["op"] not in sm.DEVICE_KINDS:
            run = []
            continue
        if "stream" in op and op["op"] != "batch_fence":
            slots = set(sm.touched(op, 0))   # (every device op with a stream names its maps)
            for kind, stream, other in run:
                if stream != op["stream"] and slots & other:
                    pairs.add((kind, op["op"]))
            run.append((op["op"], op["stream"], slots))
    return pairs


@functools.lru_cache(maxsize=None)
def all_ordered_pairs():
    return frozenset(p for shape, seed in CASES for p in ordered_pairs(sequence(shape, seed)))


@pytest.mark.parametrize("reader", sm.NEW_READERS)
def test_every_reader_follows_and_precedes_a_writer_of_its_map_on_another_stream(reader):
    pairs = all_ordered_pairs()
    assert any((w, reader) in pairs for w in sm.MUTATING_DEVICE_KINDS), f"no read after write for {reader}"
    assert any((reader, w) in pairs for w in sm.MUTATING_DEVICE_KINDS), f"no write after read for {reader}"


def test_the_import_follows_and_precedes_batches_and_exports_of_its_map_on_another_stream():
    pairs = all_ordered_pairs()
    for other in ("filter_batch", "export_layers"):
        assert (other, "import_layers") in pairs and ("import_layers", other) in pairs, other


def longest_run_of_device_calls(ops):
    """the longest run of ops of sm.NEW_KINDS and sm.PLANE_KINDS (argument errors apart: they take no ring entry) with nothing between
    them: (length, kinds, streams)"""
    best, run = (0, set(), set()), []
    for op in ops + [{"op": "checkpoint"}]:
        if op["op"] in sm.NEW_KINDS + sm.PLANE_KINDS and "expect" not in op:
            run.append(op)
            continue
        if len(run) > best[0]:
            best = (len(run), {o["op"] for o in run}, {o["stream"] for o in run})
        run = []
    return best


def test_one_run_of_device_calls_takes_every_entry_of_the_shared_ring_again():
    runs = [longest_run_of_device_calls(sequence(shape, seed)) for shape, seed in CASES]
    assert any(n > sm.PARAM_RING and len(kinds) >= 3 and len(streams) >= 2 for n, kinds, streams in runs), runs
    # ... and in every sequence, in one run on two caller streams, every entry by a plane kind and again by another kind
    for shape, seed in CASES:
        assert any(goes_round_the_ring(r) for r in runs_on_two_caller_streams(sequence(shape, seed))), (shape, seed)


@pytest.mark.parametrize("kind", sm.CLOUD_KINDS)
def test_every_cloud_call_occurs_chained_and_foreign(kind):
    modes, across = set(), 0
    for shape, seed in CASES:
        ops = sequence(shape, seed)
        for at, op in enumerate(ops):
            if op["op"] == kind:
                src = op["source"]
                modes.add(src["mode"])
                if src["mode"] == "chained":   # (the second generator stream names a batch by its index in the list without the third's ops)
                    src = dict(src, batch=src["batch"] if src.get("full") else sm.mid_indices(ops)[src["batch"]])
                    batch = ops[src["batch"]]
                    assert batch["op"] == "filter_batch" and batch["slots"][src["row0"]: src["row0"] + len(op["slots"])] == op["slots"]
                    assert ("masks" if op["masks"] else "labels") in batch["outputs"]
                    assert not any(o["op"] == "checkpoint" for o in ops[src["batch"]: at]), "the batch's buffers are gone"
                    across += batch["stream"] != op["stream"]
                else:   # the header's preconditions
                    assert len(set(op["slots"])) == len(op["slots"]) == len(src["clouds"])
                    assert all((0 if c["kind"] == "empty" else c["n"]) <= src["stride"] <= sm.SHAPES[shape]["stride"] for c in src["clouds"])
                    assert not op["masks"] or src["stride"] % 4 == 0
    assert modes == {"chained", "foreign"}, (kind, modes)
    assert across >= 1, f"{kind} never reads the labels of a batch on another stream"


# ---------------------------------------------------------------------------------------------------------------- the calls on caller-held planes

# length and digest (as above) of every committed list as it was before the third generator stream's ops were inserted
BEFORE_THE_PLANE_CALLS = {
    ("latency", 0): (198, "9f692db75a1f651586bba06528f4f9ab"),
    ("latency", 1): (198, "7848a27c641b5e9e10601c382a621805"),
    ("fleet", 0): (368, "a7510db42e99f09af022e2ad55063545"),
    ("fleet", 1): (341, "7fe47bddfd500b604d2f695e3525d786"),
    ("server", 0): (204, "dea37734b6ac68173b8943a02dd224e3"),
    ("server", 1): (196, "a3ded0ee8d89f556693b32d42ed6d353"),
}
CALLER_STREAMS = ("s1", "s2", "default")


def plane_ops(shape=None):
    """(shape, seed, index, op, list) of every plane op of the committed sequences that is no argument error"""
    for sh, seed in CASES:
        if shape in (None, sh):
            ops = sequence(sh, seed)
            for i, op in enumerate(ops):
                if op["op"] in sm.PLANE_KINDS and "expect" not in op:
                    yield sh, seed, i, op, ops


def chained_inputs(op):
    return {name: src for name, src in sp.sources_of(op).items() if sp.is_chained(src)}


def last_checkpoint(ops, i):
    return max((j for j in range(i) if ops[j]["op"] == "checkpoint"), default=-1)


def test_the_committed_seeds_keep_every_op_they_had_before_the_plane_calls():
    """make_sequence(.., plane_calls=False) is the list from before the plane calls were added, dict for dict, and a subsequence of the
    full list; the third generator stream's ops are the ones that carry "g3", and every op of a plane kind is one of them"""
    for shape, seed in CASES:
        mid = sm.make_sequence(seed, shape, plane_calls=False)
        assert (len(mid), hashlib.sha256(json.dumps(mid, sort_keys=True).encode()).hexdigest()[:32]) == BEFORE_THE_PLANE_CALLS[(shape, seed)], (shape, seed)
        full = sequence(shape, seed)
        assert [op for op in full if "g3" not in op] == mid
        assert all("g3" in op for op in full if op["op"] in sm.PLANE_KINDS) and not any(op["op"] in sm.PLANE_KINDS for op in mid)
        assert [op["g3"] for op in full if "g3" in op] == list(range(len(full) - len(mid)))


def test_every_plane_call_occurs_in_every_shape_on_every_kind_of_stream_chained_and_foreign():
    for shape in sm.SHAPES:
        seen = {op["op"] for _, _, _, op, _ in plane_ops(shape)}
        assert seen == set(sm.PLANE_KINDS), (shape, set(sm.PLANE_KINDS) - seen)
    for kind in sm.PLANE_KINDS:
        mine = [op for _, _, _, op, _ in plane_ops() if op["op"] == kind]
        streams = {op["stream"] for op in mine}
        assert streams & {"s1", "s2"} and {"default", "ctx"} <= streams, (kind, streams)
        assert any(chained_inputs(op) for op in mine), f"{kind} never reads what an earlier op wrote"
        assert any(not chained_inputs(op) for op in mine), f"{kind} never reads planes that belong to no call"
        assert {op["row_major"] for op in mine} == {False, True} and {bool(op["pad"]) for op in mine} == {False, True}, kind
    # every nullable output is left out somewhere, and given somewhere
    for kind, names in (("fuse_states", ["fused", "frontier", "counts"]), ("route_planes", ["next", "counts"]), ("footprint_planes", ["mask", "fit", "counts"]),
                        ("route_headings", ["next", "best", "best_heading", "counts"])):
        wants = [set(op["want"]) for _, _, _, op, _ in plane_ops() if op["op"] == kind]
        for name in names:
            assert any(name in w for w in wants) and any(name not in w for w in wants), (kind, name)
    for kind, key in (("route_planes", "starts"), ("route_headings", "starts"), ("match_planes", "pivots"), ("match_planes", "angles"), ("route_planes", "blocked"),
                      ("route_planes", "cost"), ("route_headings", "cost"), ("fuse_states", "evidence_in"), ("fuse_states", "shifts"), ("track_clusters", "prev")):
        given = {op[key] is not None for _, _, _, op, _ in plane_ops() if op["op"] == kind}
        assert given == {False, True}, (kind, key)
    assert {op["scores"] for _, _, _, op, _ in plane_ops() if op["op"] == "match_planes"} == {False, True}
    assert {op["cell_track"] for _, _, _, op, _ in plane_ops() if op["op"] == "track_clusters"} == {False, True}
    assert {op["M"] for _, _, _, op, _ in plane_ops() if op["op"] == "track_clusters"} == {1, 3, 64, 1024}
    assert {op["gate"] for _, _, _, op, _ in plane_ops() if op["op"] == "track_clusters"} == {0, 1, 2, 3, 4}
    # the sizes the issue keeps small
    for shape, _, _, op, _ in plane_ops():
        k = op["op"]
        assert k not in ("footprint_planes", "route_headings") or op["K"] <= (4 if shape == "latency" else 8)
        assert k != "footprint_planes" or op["radius"] <= 3
        assert k != "match_planes" or (op["window"] <= 4 and (op["angles"] is None or len(op["angles"]) <= 8))
        assert k != "track_clusters" or op["M"] < 1024 or op["n"] <= 2


def test_every_chain_the_header_names_occurs_and_a_chained_plane_keeps_its_producer_s_order():
    seen = {key: set() for key in sp.CHAIN_TABLE}
    for _, _, i, op, ops in plane_ops():
        for name, src in chained_inputs(op).items():
            made = ops[src["op"]]
            assert src["op"] < i and not (made["op"] in sm.PLANE_KINDS and "expect" in made)
            assert made["row_major"] == op["row_major"], "a chained plane is taken in the order it was written in"
            assert (made["n"] if made["op"] in sm.PLANE_KINDS else len(made["slots"])) >= src["row0"] + op["n"]
            seen[(op["op"], name)].add(src["out"])
    assert seen == sp.CHAIN_TABLE, {k: sp.CHAIN_TABLE[k] - v for k, v in seen.items() if sp.CHAIN_TABLE[k] - v}


@pytest.mark.parametrize("kind", sm.PLANE_KINDS)
def test_every_plane_call_reads_what_an_op_on_another_stream_wrote_since_the_last_checkpoint(kind):
    found = 0
    for _, _, i, op, ops in plane_ops():
        if op["op"] == kind:
            cp = last_checkpoint(ops, i)
            found += any(src["op"] > cp and ops[src["op"]]["stream"] != op["stream"] for src in chained_inputs(op).values())
    assert found, kind


def overwrites_what_another_stream_read(ops, i):
    """does plane op i write a chain buffer that an earlier op on another stream has read since the last checkpoint?"""
    op = ops[i]
    outs = {"fuse_states": ("evidence",), "track_clusters": ("tracks", "heads")}[op["op"]]
    if op.get("chain") is None:
        return False
    for j in range(last_checkpoint(ops, i) + 1, i):
        other = ops[j]
        if other["op"] in sm.PLANE_KINDS and other["stream"] != op["stream"]:
            for src in chained_inputs(other).values():
                made = ops[src["op"]]
                if src["out"] in outs and made["op"] == op["op"] and (made.get("chain"), made.get("buf")) == (op["chain"], op["buf"]):
                    return True
    return False


@pytest.mark.parametrize("kind", ["fuse_states", "track_clusters"])
def test_a_chain_s_buffer_is_overwritten_while_a_call_on_another_stream_may_still_read_it(kind):
    assert any(overwrites_what_another_stream_read(ops, i) for _, _, i, op, ops in plane_ops() if op["op"] == kind), kind


def test_a_chain_buffer_is_written_once_between_two_checkpoints():
    """... so that what every call wrote can still be compared at the checkpoint"""
    for shape, seed in CASES:
        written = set()
        for op in sequence(shape, seed):
            if op["op"] == "checkpoint":
                written = set()
            elif op["op"] in ("fuse_states", "track_clusters") and op.get("chain") is not None:
                key = (op["op"], op["chain"], op["buf"])
                assert key not in written, (shape, seed, key)
                written.add(key)


RING_TAKERS = set(sm.NEW_KINDS) | set(sm.PLANE_KINDS) | set(sm.LATE_KINDS) | {"export_layers"}   # (gg_context.hip: the calls that go through map_call_begin)


def runs_on_two_caller_streams(ops):
    """the maximal runs of device ops on caller streams (nothing in them synchronises the host: no op on the context's own stream, for
    which the driver waits for its own uploads)"""
    runs, run = [], []
    for op in ops + [{"op": "checkpoint"}]:
        if op["op"] in sm.DEVICE_KINDS and op.get("stream") in CALLER_STREAMS and "expect" not in op:
            run.append(op)
        else:
            if run:
                runs.append(run)
            run = []
    return [r for r in runs if len({op["stream"] for op in r}) == 2]


def goes_round_the_ring(run, kinds=tuple(sm.PLANE_KINDS)):
    """every entry of the ring is taken by a plane kind (by one of `kinds`) and later by another kind"""
    takers = [op["op"] for op in run if op["op"] in RING_TAKERS]
    for e in range(sm.PARAM_RING):
        mine = takers[e:: sm.PARAM_RING]
        if not any(a in kinds and any(b != a for b in mine[k + 1:]) for k, a in enumerate(mine)):
            return False
    return True


def test_one_run_per_sequence_holds_the_six_plane_kinds_on_two_caller_streams_and_goes_round_the_ring():
    for shape, seed in CASES:
        good = [r for r in runs_on_two_caller_streams(sequence(shape, seed))
                if len(r) >= 7 and set(sm.PLANE_KINDS) <= {op["op"] for op in r} and {op["op"] for op in r} & {"filter_batch", "move_maps", "export_layers"}]
        assert good, (shape, seed)
        assert any(goes_round_the_ring(r) for r in good), (shape, seed, "the same run goes round the ring")


def moves_since(ops, i, spec):
    """per slot of a shift spec, how many moves of it stand between the chain's previous observation and op i"""
    out = []
    for s in spec["of"]:
        out.append(sum(1 for j in range(spec["since"] + 1, i)
                       if (ops[j]["op"] == "move_maps" and s in ops[j]["slots"]) or (ops[j]["op"] == "map_move" and ops[j]["slot"] == s)))
    return out


@pytest.mark.parametrize("kind", sp.SHIFTED_KINDS)
def test_the_shifts_of_a_chain_are_sums_of_several_moves_end_with_a_reset_and_reach_a_side(kind):
    """For fuse and tracks "behind a reset" is behaviour: the call has no prior and names what it lost, which the mutant that lets a prior
    survive takes instead.  gg_match_planes has no prior of its own: behind a reset it stands behind the chain's first fuse, reads that
    call's evidence with no shift, and carries an empty "lost" as a MARK only -- no mutant can be told at such an op."""
    several = lost = far = 0
    for shape, seed, i, op, ops in plane_ops():
        if op["op"] != kind:
            continue
        lost += "lost" in op
        if op["shifts"] is not None:
            if "since" in op["shifts"]:
                several += max(moves_since(ops, i, op["shifts"])) >= 2
            far += any(max(abs(a), abs(b)) >= sp.side_of(sm, shape) for a, b in truth(shape, seed)[3][i]["_shifts"])
    assert several and lost and far, (kind, several, lost, far)


def test_a_reset_of_a_chain_s_slot_stands_in_front_of_every_call_that_names_what_it_lost():
    for _, _, i, op, ops in plane_ops():
        if "lost" in op and op["op"] != "match_planes":
            since, of = op["lost"]["shifts"]["since"], op["lost"]["shifts"]["of"]
            assert any(o["op"] in ("reset_maps", "map_reset", "set_position") and set(sm.touched(o, 0)) & set(of) for o in ops[since:i]), (i, op["op"])
            assert all(op[name] is None for name in op["lost"] if name != "shifts"), "no prior"


def test_at_most_a_tenth_of_the_shifted_plane_calls_have_an_all_zero_shift():
    total = still = 0
    for shape, seed, i, op, _ in plane_ops():
        if op["op"] in sp.SHIFTED_KINDS and op["shifts"] is not None:
            total += 1
            still += not any(a or b for a, b in truth(shape, seed)[3][i]["_shifts"])
    assert total > 60 and still <= 0.10 * total, (still, total)


def test_at_most_a_tenth_of_the_routes_have_nowhere_to_go_and_of_the_tracks_no_predecessor():
    for kinds in (("route_planes", "route_headings"), ("track_clusters",)):
        total = inert = 0
        for shape, seed, i, op, _ in plane_ops():
            if op["op"] in kinds:
                total += 1
                inert += not any(truth(shape, seed)[3][i]["_live"])
        assert total > 40 and inert <= 0.10 * total, (kinds, inert, total)
    # the track calls on a chain's own id planes alone, foreign ones apart.  A call without a prior cannot have a predecessor (the header:
    # Kp = 0), so the cap is over those that have one
    total = inert = 0
    for shape, seed, i, op, _ in plane_ops():
        if op["op"] == "track_clusters" and sp.is_chained(op["cells"]) and op["prev"] is not None:
            total += 1
            inert += not any(truth(shape, seed)[3][i]["_live"])
    assert total >= 10 and inert <= 0.10 * total, ("chained tracks with a prior", inert, total)


def test_once_per_shape_a_call_fills_the_rows_to_the_last_and_one_map_more_is_refused():
    for shape in sm.SHAPES:
        n_slots = sm.SHAPES[shape]["n_slots"]
        full = {op["op"]: op for _, _, _, op, _ in plane_ops(shape) if op["n"] == n_slots}
        assert {"fuse_states", "route_planes"} <= set(full), (shape, set(full))
        sh = full["fuse_states"]["shifts"]["values"]
        st = full["route_planes"]["starts"]
        assert len({tuple(v) for v in sh}) == n_slots, "another shift for every map of the call"
        assert all(sh[i] != sh[i + 1] for i in range(n_slots - 1)) and all(st[i] != st[i + 1] or st[i] is None for i in range(n_slots - 1))
        refused = 0
        for seed in SEEDS[shape]:
            ops = sequence(shape, seed)
            for i, op in enumerate(ops):
                if "expect" in op:
                    assert op["n"] == n_slots + 1 and op["expect"] == "GG_ERR_CAPACITY"
                    nxt = ops[i + 1]   # (the op behind it shows that the refused call took no ring entry and left no event behind)
                    assert nxt["op"] == op["op"] and "expect" not in nxt and nxt["stream"] == op["stream"]
                    refused += 1
        assert refused, shape


# ---------------------------------------------------------------------------------------------------------------- box_clusters, score_rollouts, clearance_planes

# length and digest (as above) of every committed list as it was before the fourth generator stream's ops were inserted
BEFORE_THE_LATE_CALLS = {
    ("latency", 0): (230, "7f090c3d5b8cb47e90cfc27b168a7848"),
    ("latency", 1): (231, "a8edbac1193d413d443638a9c35687c9"),
    ("fleet", 0): (462, "74385f3ed659de8dac13340815b04a09"),
    ("fleet", 1): (454, "e0317c5f7a724d873b605d5ebd4c928b"),
    ("server", 0): (275, "ece77dd4cb93729ca53f5245a09dc3f7"),
    ("server", 1): (310, "e74b7bccd63b4c39bc0af17e65c1fbe2"),
}
POSITION_WRITERS = ("move_maps", "reset_maps")


def late_ops(shape=None, kind=None):
    """(shape, seed, index, op, list) of every op of sm.LATE_KINDS of the committed sequences that is no argument error"""
    for sh, seed in CASES:
        if shape in (None, sh):
            ops = sequence(sh, seed)
            for i, op in enumerate(ops):
                if op["op"] in sm.LATE_KINDS and "expect" not in op and kind in (None, op["op"]):
                    yield sh, seed, i, op, ops


def test_the_committed_seeds_keep_every_op_they_had_before_the_late_calls():
    """make_sequence(.., late_calls=False) is the list from before the three calls were added, dict for dict; the fourth generator stream's
    ops are the ones that carry "g4", every op of a late kind is one of them, and they stand behind every other op but the last checkpoint:
    in front of its tail the stream adds nothing"""
    for shape, seed in CASES:
        old = sm.make_sequence(seed, shape, late_calls=False)
        assert (len(old), hashlib.sha256(json.dumps(old, sort_keys=True).encode()).hexdigest()[:32]) == BEFORE_THE_LATE_CALLS[(shape, seed)], (shape, seed)
        full = sequence(shape, seed)
        assert [op for op in full if "g4" not in op] == old
        assert all("g4" in op for op in full if op["op"] in sm.LATE_KINDS) and not any(op["op"] in sm.LATE_KINDS for op in old)
        assert [op["g4"] for op in full if "g4" in op] == list(range(len(full) - len(old)))
        assert full[: len(old) - 1] == old[:-1] and full[-1] == old[-1] == {"op": "checkpoint"}


def test_every_late_call_occurs_in_every_shape_on_every_kind_of_stream_chained_and_foreign():
    for shape in sm.SHAPES:
        seen = {op["op"] for _, _, _, op, _ in late_ops(shape)}
        assert seen == set(sm.LATE_KINDS), (shape, set(sm.LATE_KINDS) - seen)
    for kind in sm.LATE_KINDS:
        mine = [op for _, _, _, op, _ in late_ops(kind=kind)]
        streams = {op["stream"] for op in mine}
        assert streams & {"s1", "s2"} and {"default", "ctx"} <= streams, (kind, streams)
        for name in sl.INPUTS[kind]:   # every input occurs chained, and foreign
            given = [op[name] for op in mine if op[name] is not None]
            assert any(sp.is_chained(src) for src in given) and any(not sp.is_chained(src) for src in given), (kind, name)
    boxes = [op for _, _, _, op, _ in late_ops(kind="box_clusters")]
    assert {op["criterion"] for op in boxes} == {"area", "edge"} and {op["costs"] for op in boxes} == {False, True}
    assert {op["slot_list"] for op in boxes} == {False, True}
    assert {(op["source"]["fmt"], op["source"]["tfs"] is not None) for op in boxes if op["source"]["mode"] == "foreign"} == {(16, False), (16, True), (32, False), (32, True)}
    assert any(op["source"]["mode"] == "chained" for op in boxes)
    rolls = [op for _, _, _, op, _ in late_ops(kind="score_rollouts")]
    assert {op["row_major"] for op in rolls} == {False, True} and {bool(op["pad"]) for op in rolls} == {False, True}
    assert {op["relative"] for op in rolls} == {False, True} and {op["best"] for op in rolls} == {False, True}
    for name in ("cost", "dist", "clear"):
        assert {op[name] is not None for op in rolls} == {False, True}, name
    assert {op["reach"] for op in rolls} == {0, 1, 63}
    pads = {op["table"]["pad"] for op in rolls if op["n"] >= 2}
    assert 0 in pads and any(p % 2 for p in pads), "a shared table, and per-map tables an odd number of words apart"
    assert all(not op["table"]["pad"] or (4 * op["table"]["P"] * op["table"]["T"] + op["table"]["pad"]) % 2 for op in rolls)
    assert any(None in op["starts"] and any(s is not None for s in op["starts"]) for op in rolls), "a map without a start among maps with one"
    clears = [op for _, _, _, op, _ in late_ops(kind="clearance_planes")]
    assert {op["row_major"] for op in clears} == {False, True} and {bool(op["pad"]) for op in clears} == {False, True}
    for key in ("nearest", "distance", "count"):
        assert {op[key] for op in clears} == {False, True}, key


def test_the_late_calls_stay_small():
    """the references are plain loops"""
    big = {shape: 0 for shape in sm.SHAPES}
    for shape in sm.SHAPES:
        assert set(sl.ROLLOUT_P) <= {op["table"]["P"] for _, _, _, op, _ in late_ops(shape, "score_rollouts")}, shape
        assert {op["M"] for _, _, _, op, _ in late_ops(shape, "box_clusters")} <= set(sl.BOX_M)
    for shape, _, _, op, _ in late_ops():
        if op["op"] == "score_rollouts":
            P, T = op["table"]["P"], op["table"]["T"]
            assert op["K"] <= (4 if shape == "latency" else 8) and 1 <= T <= 12 and P * T <= 4096
            if P == 1025:
                assert T <= 3 and op["n"] <= 2
                big[shape] += 1
            else:
                assert P <= 1024
        elif op["op"] == "box_clusters":
            assert op["M"] in sl.BOX_M and op["K"] in sl.BOX_K
    assert all(v == 1 for v in big.values()), big   # (the stride loop of 1024 threads: once per shape)
    assert {op["M"] for _, _, _, op, _ in late_ops(kind="box_clusters")} == set(sl.BOX_M)
    assert {op["K"] for _, _, _, op, _ in late_ops(kind="box_clusters")} == set(sl.BOX_K)


def test_every_late_chain_occurs_and_a_chained_buffer_is_taken_as_its_producer_left_it():
    seen = {key: set() for key in sl.CHAIN_TABLE}
    clear_made_by = set()
    for _, _, i, op, ops in late_ops():
        for name, src in sl.chained_inputs(op).items():
            made = ops[src["op"]]
            assert src["op"] < i and "expect" not in made
            assert (made["n"] if "n" in made else len(made["slots"])) >= src["row0"] + op["n"]
            seen[(op["op"], name)].add(src["out"])
            if op["op"] == "box_clusters":   # the cluster call's ids and counts, on that call's points and maps, while its buffers are there
                assert made["op"] == "cluster_clouds" and made["point_clusters"] and op["n_clusters"]["op"] == op["point_cluster"]["op"]
                assert made["slots"] == op["slots"] and made["source"] == op["source"]
                assert last_checkpoint(ops, i) < src["op"]
            else:
                assert made["row_major"] == op["row_major"], "a chained plane is taken in the order it was written in"
            if name == "dist":
                assert made["op"] == "route_headings" and made["K"] == op["K"]
            if name == "clear":
                clear_made_by.add(made["op"])
        if op["op"] == "box_clusters" and op["source"]["mode"] == "chained":
            assert last_checkpoint(ops, i) < op["source"]["batch"], "the batch's buffers are gone"
    assert seen == sl.CHAIN_TABLE, {k: sl.CHAIN_TABLE[k] - v for k, v in seen.items() if sl.CHAIN_TABLE[k] - v}
    assert clear_made_by == sl.CLEAR_PRODUCERS, clear_made_by
    # a box call reads a cluster call of its batch's clouds, and one of clouds that belong to no batch
    assert {op["source"]["mode"] for _, _, _, op, _ in late_ops(kind="box_clusters") if sl.chained_inputs(op)} == {"chained", "foreign"}


def test_the_foreign_inputs_of_the_late_calls_hold_what_the_header_says_is_safe():
    ids = np.concatenate([sl.foreign_ids(dict(seed=s), 0, 400, 3) for s in range(5)])
    assert (ids < -1).any() and (ids == sl.I32_MIN).any() and (ids >= 3).any() and ((ids >= 0) & (ids < 3)).mean() > 0.7
    counts = [sl.foreign_count(dict(seed=0), i, 64) for i in range(7)]
    assert min(counts) < 0 and max(counts) > 64 and 64 in counts
    vol = sl.dist_volume(dict(seed=3, kind="evidence", distinct=4), 1, 4, 79)
    assert vol.shape == (4, 79, 79) and (vol == sl.NONE).any() and (vol < 0).any() and (vol > 0).any()
    used = False
    for _, _, _, op, _ in late_ops(kind="box_clusters"):
        used |= not sp.is_chained(op["point_cluster"]) and not sp.is_chained(op["n_clusters"])
    assert used



@pytest.mark.parametrize("kind", sm.LATE_KINDS)
def test_every_late_call_reads_what_an_op_on_another_stream_wrote_since_the_last_checkpoint(kind):
    found = 0
    for _, _, i, op, ops in late_ops(kind=kind):
        cp = last_checkpoint(ops, i)
        found += any(src["op"] > cp and ops[src["op"]]["stream"] != op["stream"] for src in sl.chained_inputs(op).values())
    assert found, kind


def test_the_box_call_follows_and_precedes_a_position_writer_of_its_map_on_another_stream():
    pairs = all_ordered_pairs()
    for w in POSITION_WRITERS:
        assert (w, "box_clusters") in pairs, f"no box call behind a {w} of its map on another stream"
    assert any(("box_clusters", w) in pairs for w in POSITION_WRITERS), "no position writer behind a box call on another stream"
    assert ("box_clusters", "move_maps") in pairs
    # ... and a move of one of its maps stands between the cluster call and the box call that reads it
    between = 0
    for _, _, i, op, ops in late_ops(kind="box_clusters"):
        if sp.is_chained(op["point_cluster"]):
            between += any(o["op"] == "move_maps" and set(o["slots"]) & set(op["slots"]) and o["stream"] != op["stream"] for o in ops[op["point_cluster"]["op"]: i])
    assert between >= len(CASES)


def test_one_run_per_sequence_holds_more_rollout_calls_than_the_ring_has_entries():
    """... on two caller streams with nothing that synchronises the host: their starts differ pairwise (each travels in its ring entry),
    other ring takers stand between them, and every entry is taken by a late kind and later by another kind"""
    for shape, seed in CASES:
        good = 0
        for run in runs_on_two_caller_streams(sequence(shape, seed)):
            takers = [op for op in run if op["op"] in RING_TAKERS]
            at = [k for k, op in enumerate(takers) if op["op"] == "score_rollouts"]
            starts = [json.dumps(takers[k]["starts"]) for k in at]
            good += (len(at) > sm.PARAM_RING and len(set(starts)) == len(starts) and all(b - a >= 2 for a, b in zip(at, at[1:]))
                     and goes_round_the_ring(run, tuple(sm.LATE_KINDS)) and set(sm.LATE_KINDS) <= {op["op"] for op in run})
        assert good, (shape, seed)


def test_a_distance_buffer_is_overwritten_while_a_rollout_call_on_another_stream_may_still_read_it():
    for shape, seed in CASES:
        ops = sequence(shape, seed)
        hit, written = 0, set()
        for i, op in enumerate(ops):
            if op["op"] == "checkpoint":
                written = set()
            if op["op"] != "clearance_planes" or op.get("buf") is None or "expect" in op:
                continue
            key = (op["buf"], op["n"], op["pad"])
            assert key not in written, (shape, seed, i, "written twice between two checkpoints")
            written.add(key)
            for j in range(last_checkpoint(ops, i) + 1, i):
                other = ops[j]
                src = other.get("clear") if other["op"] == "score_rollouts" else None
                if sp.is_chained(src) and other["stream"] != op["stream"]:
                    made = ops[src["op"]]
                    hit += made["op"] == "clearance_planes" and (made.get("buf"), made["n"], made["pad"]) == key and src["op"] < last_checkpoint(ops, i)
        assert hit, (shape, seed)


def test_every_predicate_meets_every_late_kind_dealt_over_the_six_sequences():
    dealt = [pair for shape, seed in CASES for pair in sl._late_pairs(sm, shape, seed)]
    assert sorted(dealt) == sorted((p, k) for p in sm.PREDICATES for k in sm.LATE_KINDS)
    table = coverage_table()
    assert all(table[p][k] > 0 for p in sm.PREDICATES for k in sm.LATE_KINDS)


def test_once_per_shape_and_late_kind_a_call_names_n_slots_maps_and_one_map_more_is_refused():
    for shape in sm.SHAPES:
        n_slots = sm.SHAPES[shape]["n_slots"]
        full = {op["op"] for _, _, _, op, _ in late_ops(shape) if op["n"] == n_slots}
        assert full == set(sm.LATE_KINDS), (shape, full)
        refused = []
        for seed in SEEDS[shape]:
            ops = sequence(shape, seed)
            for i, op in enumerate(ops):
                if "expect" in op and op["op"] in sm.LATE_KINDS:
                    assert op["n"] == n_slots + 1 and op["expect"] == "GG_ERR_CAPACITY" and op.get("buf") is None
                    assert ops[i - 1]["op"] == op["op"] and ops[i - 1]["n"] == n_slots and ops[i - 1]["stream"] == op["stream"] != "ctx"
                    assert ops[i + 1]["op"] == op["op"] and "expect" not in ops[i + 1] and ops[i + 1]["stream"] == op["stream"]   # (inside a run)
                    refused.append(op["op"])
        assert sorted(refused) == sorted(sm.LATE_KINDS), (shape, refused)


@pytest.mark.parametrize("kind", sm.LATE_KINDS)
def test_at_most_a_tenth_of_the_late_calls_are_inert(kind):
    """a box call without a participating point in any cloud, a rollout call whose best p is -1 in every map, a clearance call without a seed"""
    total = inert = 0
    for shape, seed, i, op, _ in late_ops(kind=kind):
        total += 1
        inert += not any(truth(shape, seed)[3][i]["_live"])
    assert total >= 30 and inert <= 0.10 * total, (kind, inert, total)


def test_the_lazy_layer_mutant_trips_on_every_late_kind():
    tripped = set()
    for shape, seed in CASES:
        results = truth(shape, seed)[0]
        model = sm.ContextModel(shape, mutant="plane_call_computes_lazy_layers").bind(sequence(shape, seed))
        for i, op in enumerate(sequence(shape, seed)):
            got = model.apply(op, i)
            if op["op"] in sm.LATE_KINDS and differs(results[i], got):
                tripped.add(op["op"])
    assert tripped == set(sm.LATE_KINDS), tripped


# ---------------------------------------------------------------------------------------------------------------- inertness caps

def test_at_most_a_tenth_of_the_filter_ops_have_no_point_inside_the_map():
    total = inert = 0
    for shape, seed in CASES:
        per_op = {}
        for i, n in truth(shape, seed)[2]:
            per_op[i] = per_op.get(i, 0) + n
        total += len(per_op)
        inert += sum(1 for n in per_op.values() if n == 0)
    assert total > 100 and 0 < inert <= 0.10 * total, (inert, total)


def test_at_most_a_tenth_of_the_moves_have_shift_zero():
    """counted per moved map, not per call"""
    total = still = 0
    for shape, seed in CASES:
        for op, res in zip(sequence(shape, seed), truth(shape, seed)[0]):
            if op["op"] in ("move_maps", "map_move"):
                shifts = (res["shifts"] if op["op"] == "move_maps" else res["shift"]).reshape(-1, 2)
                total += len(shifts)
                still += int((~shifts.any(axis=1)).sum())
    assert total > 100 and 0 < still <= 0.10 * total, (still, total)


def test_the_server_shape_divides_batches_with_and_without_a_fence_behind_them():
    """GG_FLAG_CONCURRENT_HALVES at the default threshold: a batch of more than 256 clouds on a caller stream, the next batch on another
    stream right behind it -- once with gg_batch_fence between the two, once without"""
    seen = set()
    for seed in SEEDS["server"]:
        ops, halves = sequence("server", seed), False
        for i, op in enumerate(ops):
            if op["op"] == "set_flags":
                halves = op["halves"]
            if op["op"] == "filter_batch" and halves and len(op["slots"]) > 256 and op["stream"] in ("s1", "s2"):
                nxt = ops[i + 1]
                if nxt["op"] == "batch_fence" and ops[i + 2]["op"] == "filter_batch":
                    seen.add("fenced")
                elif nxt["op"] == "filter_batch" and nxt["stream"] != op["stream"]:
                    seen.add("unfenced")
    assert seen == {"fenced", "unfenced"}, seen


@pytest.mark.parametrize("kind", sm.MUTATING)
def test_deleting_every_op_of_a_mutating_kind_changes_something_compared(kind):
    assert first_kill(drop=kind), f"no committed sequence notices that its {kind} ops are gone"


# ---------------------------------------------------------------------------------------------------------------- detection power

def test_the_true_model_agrees_with_itself():
    assert distinguishes("fleet", 0) is None


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_a_committed_seed_tells_the_mutant_from_the_true_model(mutant):
    assert first_kill(mutant=mutant), f"no committed sequence distinguishes the model with {mutant}"


# ---------------------------------------------------------------------------------------------------------------- the tables of DESIGN.md

def tables():
    t = coverage_table()
    rows = ["| op kind | any | " + " | ".join(sm.PREDICATES) + " |", "|---|" + "---|" * (1 + len(sm.PREDICATES))]
    for k in sm.KINDS:
        rows.append(f"| {k} | {t['any'][k]} | " + " | ".join(str(t[p][k]) if k in t[p] else "n/a" for p in sm.PREDICATES) + " |")
    rows += ["", "| mutant | killed by | first difference |", "|---|---|---|"]
    for m in sm.MUTANTS:
        shape, seed, d = first_kill(mutant=m) or ("-", "-", "NOT KILLED")
        rows.append(f"| {m} | {shape} seed {seed} | {d[:110]} |")
    rows += ["", "| ops of this kind deleted | noticed by |", "|---|---|"]
    for k in sm.MUTATING:
        shape, seed, d = first_kill(drop=k) or ("-", "-", "NOT NOTICED")
        rows.append(f"| {k} | {shape} seed {seed}: {d[:90]} |")
    pairs = all_ordered_pairs()
    rows += ["", "| device call | follows, on another stream, a ... of its map | is followed by | chained / foreign |", "|---|---|---|---|"]
    others = sorted(sm.MUTATING_DEVICE_KINDS | {"export_layers"})
    for k in sm.NEW_KINDS:
        modes = [op["source"]["mode"] for shape, seed in CASES for op in sequence(shape, seed) if op["op"] == k and "source" in op]
        rows.append(f"| {k} | " + ", ".join(o for o in others if (o, k) in pairs and o != k) + " | " + ", ".join(o for o in others if (k, o) in pairs and o != k)
                    + " | " + (f"{modes.count('chained')} / {modes.count('foreign')}" if modes else "n/a") + " |")
    for k in sm.PLANE_KINDS:   # (a plane call "names" slots 0 .. n - 1; chained: at least one input is an earlier op's buffer)
        mine = [op for _, _, _, op, _ in plane_ops() if op["op"] == k]
        rows.append(f"| {k} | " + ", ".join(o for o in others if (o, k) in pairs) + " | " + ", ".join(o for o in others if (k, o) in pairs)
                    + f" | {sum(1 for op in mine if chained_inputs(op))} / {sum(1 for op in mine if not chained_inputs(op))} |")
    for k in sm.LATE_KINDS:   # (a box call names its slots, the other two slots 0 .. n - 1)
        mine = [op for _, _, _, op, _ in late_ops(kind=k)]
        rows.append(f"| {k} | " + ", ".join(o for o in others if (o, k) in pairs) + " | " + ", ".join(o for o in others if (k, o) in pairs)
                    + f" | {sum(1 for op in mine if sl.chained_inputs(op))} / {sum(1 for op in mine if not sl.chained_inputs(op))} |")
    n, kinds, streams = max((longest_run_of_device_calls(sequence(shape, seed)) for shape, seed in CASES), key=lambda r: r[0])
    rows += ["", f"longest run of device calls: {n} ops of {len(kinds)} kinds on {len(streams)} streams (the shared ring has {sm.PARAM_RING} entries)"]
    return "\n".join(rows)


if __name__ == "__main__":
    print(tables())
