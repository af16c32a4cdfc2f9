"""Seeded sequences of API calls on the device, held op by op to the per-slot oracle model of tests/seq_model.py.

One test per (context shape, seed).  Outputs of device ops are compared only at the sequence's checkpoints (gg_batch_fence on every caller
stream used, one synchronisation), so the library's own cross-stream ordering is what has to make them right; at the end every slot's
eleven layers, position, reported configuration and counters are compared.  A mismatch stops the sequence at that op and leaves the op
list up to it as JSON under tmp_path: replay(path, shape) runs such a prefix again in-process.

After a GG_ERR_HIP, a pending gg_device_error or any other exception than a failed comparison out of the device section (a torch
RuntimeError from a synchronisation or a copy is how a fault usually shows) the remaining tests of this file skip themselves and the
context is left alone: nothing more is started on the card.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import seq_model as sm  # noqa: E402
from tests.test_sequences_cpu import SEEDS  # noqa: E402

pytestmark = pytest.mark.gpu

_FAULT = {"what": None}   # set once by the first device fault of this file


def brief(op):
    """an op record short enough for an assertion message"""
    out = {}
    for k, v in op.items():
        if isinstance(v, list) and len(v) > 8:
            out[k] = f"[{len(v)} items, first {v[:3]}]"
        else:
            out[k] = v
    return out


def run_sequence(ops, shape, tmp_path, tag, mutant=None):
    """`ops` on a new context of `shape` against the model (`mutant`: a deliberately wrong model, to see the harness fail)"""
    if _FAULT["what"]:
        pytest.skip(f"an earlier sequence faulted the device ({_FAULT['what']}): nothing more is started on it from this file")
    model = sm.ContextModel(shape, mutant=mutant)
    want = model.run(ops)
    seg = sm.create_context(shape)
    seen = []

    def on_result(i, got):
        seen.append(i)
        d = sm.first_diff(want[i], got if got is not None else {})
        if d:
            path = os.path.join(str(tmp_path), f"{tag}_prefix_{i}.json")
            with open(path, "w") as f:
                json.dump(ops[: i + 1], f)
            raise AssertionError(f"{tag}: op {i} {brief(ops[i])}: {d}   (ops 0..{i} written to {path})")

    try:
        driver = sm.run_on_device(seg, ops, shape, on_result)
        assert seen == list(range(len(ops)))
        for s in range(model.n):
            d = sm.first_diff(model.state(s), driver.state(s, model.ids is not None))
            assert not d, f"{tag}: after the last op, slot {s}: {d}"
        driver.check_device()
        driver.release()
    except AssertionError:
        raise   # (a comparison failed: the card is fine)
    except BaseException as e:
        _FAULT["what"] = f"{tag}: {type(e).__name__}: {e}"
        raise
    finally:
        if not _FAULT["what"]:
            try:   # (exports and moves may still be in flight on the caller's streams: gg_synchronize does not wait for those)
                import torch

                torch.cuda.synchronize()
                seg.synchronize()
                seg.close()
            except BaseException as e:   # (not raised: it would hide the comparison that failed)
                _FAULT["what"] = f"{tag}: while closing the context: {type(e).__name__}: {e}"


def replay(path, shape, tmp_path="."):
    """run a recorded prefix again: python -c "from tests.test_sequences_gpu import replay; replay('x.json', 'fleet')" """
    with open(path) as f:
        run_sequence(json.load(f), shape, tmp_path, os.path.basename(path))


def consecutive_device_ops(ops):
    """the longest run of device ops (nothing in them synchronises the host) and the streams it uses"""
    best, run, streams = (0, set()), 0, set()
    for op in ops:
        if op["op"] in sm.DEVICE_KINDS:
            run += 1
            streams.add(op.get("stream"))
            if run > best[0] and len(streams) >= 2:
                best = (run, set(streams))
        else:
            run, streams = 0, set()
    return best


@pytest.mark.parametrize("shape,seed", [(shape, seed) for shape in sm.SHAPES for seed in SEEDS[shape]])
def test_sequence(shape, seed, tmp_path):
    ops = sm.make_sequence(seed, shape)
    run, streams = consecutive_device_ops(ops)
    assert run >= 3 and len(streams) >= 2, "every sequence holds three device ops in a row on two streams with no host synchronisation"
    run_sequence(ops, shape, tmp_path, f"{shape} seed {seed}")


# ---------------------------------------------------------------------------------------------------------------- regressions: one literal op list per finding

TUNINGS = {"op": "tunings", "graphs": 0, "halves_min_clouds": 0, "front": 0, "sweep_waves": 0, "scan_parts": 0, "move_chunk": 0, "export_variant": 0}
POSE = [0.3, 0.2, 1.5, 0.02, -0.01, 0.3, 0.95]


def test_per_call_layers_read_between_a_move_and_the_first_cloud(tmp_path):
    """reset -> move -> read `points` before any cloud.  A move scrolls ground and groundpatch only (include/groundgrid_hip.h,
    gg_move_map): the nine per-call layers read as they stood -- here their reset values in every cell, where the reference's
    grid_map::move leaves NaN in the exposed cells.  gg_move_maps and gg_move_map, the export and the getter, ground scrolled next to it."""
    ops = [TUNINGS,
           {"op": "reset_maps", "first": 0, "n": 3, "odom_z": -1.7, "pos": [1.0, -2.0], "persistent": False, "stream": "ctx"},
           {"op": "move_maps", "slots": [2, 0], "odoms": [[4.3, -2.0], [1.0, 1.63]], "poses": [POSE, POSE], "stream": "s1"},
           {"op": "export_layers", "slots": [0, 1, 2], "names": ["points", "ground", "minGroundHeight", "maxGroundHeight"], "row_major": False, "stream": "s2", "pad": 0},
           {"op": "map_move", "slot": 1, "odom": [-2.3, -5.3], "pose": POSE},
           {"op": "get_layers", "slot": 1, "names": None},
           {"op": "get_layer", "slot": 2, "layer": "points"},
           {"op": "checkpoint"}]
    want = sm.ContextModel("latency").run(ops)
    assert want[2]["shifts"].all() or want[2]["shifts"].any(axis=1).all()            # (both maps do scroll)
    assert not want[3]["map 2 (slot 2) layer points"].any() and not sm.np.isnan(want[5]["layer points"]).any()
    run_sequence(ops, "latency", tmp_path, "per-call layers after a move")
