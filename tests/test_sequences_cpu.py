"""The sequence harness of tests/seq_model.py without a GPU: the generator is deterministic, the committed seeds cover what they have to
cover, few ops are inert, and the model tells every deliberate bookkeeping slip (seq_model.MUTANTS) from the truth.  For the many-map
device calls (seq_model.NEW_KINDS): the committed seeds keep every op they had before those were inserted, every call occurs in every
shape, follows and precedes a writer of its map on another stream with no host synchronisation between them, one run of them is longer
than the ring they share, and every cloud call occurs chained to a batch (also on another stream than the batch) and foreign.

`python -m tests.test_sequences_cpu` prints the coverage table and the mutant table of DESIGN.md.
"""
import functools
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import seq_model as sm  # noqa: E402

# the committed seeds: tests/test_sequences_gpu.py runs exactly these
SEEDS = {"latency": [0, 1], "fleet": [0, 1], "server": [0, 1]}
CASES = [(shape, seed) for shape in ("fleet", "latency", "server") for seed in SEEDS[shape]]   # (cheapest model first)


@functools.lru_cache(maxsize=None)
def sequence(shape, seed):
    return sm.make_sequence(seed, shape)


@functools.lru_cache(maxsize=None)
def truth(shape, seed):
    """(results per op, state per slot, [(op index, points inside the map)] per filtered cloud) of the true model"""
    model = sm.ContextModel(shape)
    inside = []
    results = []
    for i, op in enumerate(sequence(shape, seed)):
        results.append(model.apply(op, i))
        for s in (sm.touched(op, model.n) if op["op"] in sm.FILTERS else []):
            inside.append((i, int((model.slots[s].last[0] != sm.oracle.OUTSIDE).sum())))
    return results, [model.state(s) for s in range(model.n)], inside


def differs(a, b):
    if (a is None) != (b is None):
        return "one of the two returns nothing"
    return sm.first_diff(a, b) or sm.first_diff(b, a)


def distinguishes(shape, seed, mutant=None, drop=None):
    """None, or where a wrong model (`mutant`) / the sequence without its ops of kind `drop` first differs from the truth in something the
    driver compares: an op's results, or a slot's final state"""
    results, states, _ = truth(shape, seed)
    model = sm.ContextModel(shape, mutant=mutant)
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
    """the longest run of ops of sm.NEW_KINDS with nothing between them: (length, kinds, streams)"""
    best, run = (0, set(), set()), []
    for op in ops + [{"op": "checkpoint"}]:
        if op["op"] in sm.NEW_KINDS:
            run.append(op)
            continue
        if len(run) > best[0]:
            best = (len(run), {o["op"] for o in run}, {o["stream"] for o in run})
        run = []
    return best


def test_one_run_of_device_calls_takes_every_entry_of_the_shared_ring_again():
    runs = [longest_run_of_device_calls(sequence(shape, seed)) for shape, seed in CASES]
    assert any(n > sm.PARAM_RING and len(kinds) >= 3 and len(streams) >= 2 for n, kinds, streams in runs), runs


@pytest.mark.parametrize("kind", sm.CLOUD_KINDS)
def test_every_cloud_call_occurs_chained_and_foreign(kind):
    modes, across = set(), 0
    for shape, seed in CASES:
        ops = sequence(shape, seed)
        for at, op in enumerate(ops):
            if op["op"] == kind:
                src = op["source"]
                modes.add(src["mode"])
                if src["mode"] == "chained":
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
    n, kinds, streams = max((longest_run_of_device_calls(sequence(shape, seed)) for shape, seed in CASES), key=lambda r: r[0])
    rows += ["", f"longest run of device calls: {n} ops of {len(kinds)} kinds on {len(streams)} streams (the shared ring has {sm.PARAM_RING} entries)"]
    return "\n".join(rows)


if __name__ == "__main__":
    print(tables())
