"""The four many-map calls (gg_reset_maps, gg_move_maps, gg_export_layers, gg_import_layers) and gg_filter_batch chained on ONE caller
stream without a host synchronisation in between, with GG_FLAG_CONCURRENT_HALVES off and on: every exported plane, the final layers, the
second batch's outputs, the returned shifts and the map positions are, bit for bit, what a second context computes with the one-map calls
(gg_reset_map, gg_move_map, gg_get_layers, gg_set_layer) and a gg_synchronize after each.  The chain passes more than PARAM_RING = 4 times
through the move ring (five gg_move_maps) and through the export ring (four exports and an import) while earlier copies may be in flight.
Every comparison is on bits; there is no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import api, synth  # noqa: E402
from groundgrid_amd._lib import LAYERS  # noqa: E402
from tests import test_export_layers_gpu as ex  # noqa: E402  (its helpers)

pytestmark = pytest.mark.gpu

LENGTH, RES, SIZE = 22.0, 0.33, 67  # 67 = 64 + 3 cells a side: two export blocks and an edge tile on either axis
N_SLOTS = 6                         # (the halves meet at slot 3)
MOVED = [3, 0, 5, 1, 4, 2]          # the permuted list of both gg_move_maps rounds
SRC, DST = [0, 2, 4], [5, 3, 1]     # exported from, imported into: either list has maps of both halves
LAZY = ex.LAZY
# the further exports behind the second batch: (layers, slots or None for all, row_major)
EXTRA = [(list(LAYERS), [1, 3, 5], False), (["ground", "groundpatch"], None, True), (LAZY, [4, 0], False)]
# odometry of map MOVED[i]: the first move leaves two maps where they are (zero shift: src/GroundGrid.cpp:135-137) ...
ODOM_FIRST = np.array([(0.9, -0.7), (0.0, 0.0), (1.8, 0.4), (-0.7, 1.1), (0.0, 0.0), (2.7, -1.4)])
# ... and four more follow the import, one after the other (MOVED[0] and MOVED[3] stay where the first one left them)
ODOM_STEP = np.array([(0.0, 0.0), (0.4, -0.5), (0.8, 0.0), (0.0, 0.0), (0.4, 0.0), (0.8, -0.5)])
ODOMS = [ODOM_FIRST + j * ODOM_STEP for j in range(5)]


def scene():
    """the inputs of both batches on the device: clouds of a few thousand points, the second batch's at the maps' last odometry"""
    base = [synth.hdl64_cloud(seed=3100 + k, n_az=52 + 5 * k) for k in range(N_SLOTS)]
    last = {MOVED[i]: ODOMS[-1][i] for i in range(N_SLOTS)}
    second = []
    for s in range(N_SLOTS):
        c = synth.clone_cloud(base[(s + 1) % N_SLOTS])
        c["x"] += np.float32(last[s][0])
        c["y"] += np.float32(last[s][1])
        second.append(c)
    stride = ex.stride_of(base)
    origins = [np.zeros((N_SLOTS, 3), np.float32), np.array([(last[s][0], last[s][1], 0.0) for s in range(N_SLOTS)], dtype=np.float32)]
    return {"pts": [ex.batch_points(base, stride), ex.batch_points(second, stride)], "n": [[len(c) for c in base], [len(c) for c in second]],
            "origins": origins, "base_z": np.full(N_SLOTS, -1.73), "stride": stride}


def positions(seg):
    out = np.empty((N_SLOTS, 2))
    for s in range(N_SLOTS):
        x, y = C.c_double(), C.c_double()
        assert seg._L.gg_get_map_position(seg._ctx, s, C.byref(x), C.byref(y)) == 0
        out[s] = (x.value, y.value)
    return out


def host_outputs(o):
    return o.labels.cpu().numpy(), o.out_index.cpu().numpy(), o.counts.cpu().numpy()


@pytest.fixture(scope="module")
def stepwise():
    """the same work with the one-map calls on the context's own stream, a gg_synchronize after each; computed once, never changed"""
    import torch

    sc = scene()
    torch.cuda.synchronize()
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=N_SLOTS, max_points=sc["stride"])
    assert seg.rows == seg.cols == SIZE

    def batch(k):
        o = seg.filter_batch(sc["pts"][k], sc["n"][k], sc["origins"][k], sc["base_z"])
        torch.cuda.synchronize()
        seg.synchronize()
        return host_outputs(o)

    def move(odoms):
        sh = np.zeros((N_SLOTS, 2), dtype=np.int32)
        for i, s in enumerate(MOVED):
            sh[i] = seg.map(s).move(odoms[i][0], odoms[i][1], ex.POSE)
            seg.synchronize()
        return sh

    for s in range(N_SLOTS):
        seg.map(s).reset(odom_z=0.0)
        seg.synchronize()
    batch(0)
    shifts = [move(ODOMS[0])]
    exported = {s: seg.map(s).layers() for s in SRC}
    for s, d in zip(SRC, DST):
        for name in LAYERS:
            seg.map(d).set(name, exported[s][name])
            seg.synchronize()
    for od in ODOMS[1:]:
        shifts.append(move(od))
    second = batch(1)
    final = {s: seg.map(s).layers() for s in range(N_SLOTS)}
    pos = positions(seg)
    seg.close()
    return {"scene": sc, "exported": exported, "shifts": shifts, "second": second, "final": final, "positions": pos}


@pytest.mark.parametrize("halves", [False, True])
def test_chain_on_one_caller_stream(stepwise, halves):
    import torch

    sc, poses = stepwise["scene"], [ex.POSE] * N_SLOTS
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=N_SLOTS, max_points=sc["stride"])
    if halves:
        seg.set_flags(concurrent_halves=True)
        seg.debug_set_tuning("halves_min_clouds", 2)
    seg.synchronize()
    torch.cuda.synchronize()  # (the scene's uploads ran on torch's default stream)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # no synchronisation from here to the end of the chain: the library orders the calls
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        seg.filter_batch(sc["pts"][0], sc["n"][0], sc["origins"][0], sc["base_z"])
        shifts = [seg.move_maps(ODOMS[0], poses, slots=MOVED, on_torch_stream=True)]
        planes = seg.export_layers(slots=SRC)
        seg.import_layers(planes, slots=DST)
        for od in ODOMS[1:]:
            shifts.append(seg.move_maps(od, poses, slots=MOVED, on_torch_stream=True))
        out = seg.filter_batch(sc["pts"][1], sc["n"][1], sc["origins"][1], sc["base_z"])
        extra = [seg.export_layers(names, slots=slots, row_major=rm) for names, slots, rm in EXTRA]
    torch.cuda.synchronize()
    seg.synchronize()

    assert sum(int((sh[i] == 0).all()) for sh in shifts[:1] for i in range(N_SLOTS)) == 2, "the first move has two zero shifts"
    for j, (got, want) in enumerate(zip(shifts, stepwise["shifts"])):
        assert np.array_equal(got, want), f"shifts of move {j}: {got.tolist()} != {want.tolist()}"
    assert any((sh != 0).any() for sh in shifts[1:])
    assert np.array_equal(positions(seg), stepwise["positions"])
    ex.assert_export_equals(planes.cpu().numpy(), seg, SRC, list(LAYERS), lambda s: stepwise["exported"][s], "the export in front of the import")
    labels, index, counts = host_outputs(out)
    want_labels, want_index, want_counts = stepwise["second"]
    assert np.array_equal(counts, want_counts)
    for k, nk in enumerate(sc["n"][1]):
        assert np.array_equal(labels[k, :nk], want_labels[k, :nk]), f"labels of cloud {k}"
        assert np.array_equal(index[k, :nk], want_index[k, :nk]), f"out_index of cloud {k}"
    for (names, slots, rm), got in zip(EXTRA, extra):
        ex.assert_export_equals(got.cpu().numpy(), seg, slots if slots is not None else list(range(N_SLOTS)), names, lambda s: stepwise["final"][s],
                                f"export of {'+'.join(names) if len(names) < 11 else 'all'} behind the second batch", row_major=rm)
    for s in range(N_SLOTS):
        got = seg.map(s).layers()
        for name in LAYERS:
            assert ex.same_bits(got[name], stepwise["final"][s][name]), f"slot {s} layer {name}: {int((ex.bits(got[name]) != ex.bits(stepwise['final'][s][name])).sum())} cells differ"
    seg.close()
