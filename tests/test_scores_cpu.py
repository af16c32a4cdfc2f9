"""The evaluator counters (gg_set_score_labels / gg_set_slot_scoring / gg_get_slot_scores) without a GPU: the header and the binding,
GroundEvaluator.from_device_counts against the published table, the skip_nans rule of add_cloud(points=...), and the premise the
device relies on -- a point of the returned cloud never has a NaN x or y -- held to the oracle on the hostile scenes."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from groundgrid_amd import _lib, build
from groundgrid_amd.evaluate import GROUND, LABELS, NONGROUND, GroundEvaluator
from oracle import oracle
from tests import edge_scenes as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "readme_seq00_table.json")
SCORE_SYMBOLS = ["gg_set_score_labels", "gg_set_slot_scoring", "gg_get_slot_scores", "gg_reset_slot_scores"]

PROG = r'''
#include <stdio.h>
#include <stddef.h>
#include "groundgrid_hip.h"
#if !defined(GG_HAS_SCORES) || GG_HAS_SCORES != 1
#error "GG_HAS_SCORES"
#endif
int main(void){ printf("%d %zu %d %zu %d %zu %zu\n", GG_HAS_SCORES, sizeof(gg_slot_scores), GG_ABI_VERSION, sizeof(gg_batch), GG_SCORE_MAX_LABELS,
    offsetof(gg_slot_scores, counts), sizeof(((gg_slot_scores *)0)->counts[0])); return 0; }
'''


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_header_compiles_in_c_and_cpp_with_the_scores(compiler, suffix):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t." + suffix)
        open(src, "w").write(PROG)
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")], text=True).split()]
    assert vals == [1, 8 + 65 * 2 * 8, 6, C.sizeof(_lib.GGBatch), 64, 8, 16]
    assert C.sizeof(_lib.GGBatch) == 120                       # gg_batch keeps its size
    assert C.sizeof(_lib.GGSlotScores) == 8 + 65 * 2 * 8 and _lib.GGSlotScores.counts.offset == 8
    assert _lib.GG_ABI_VERSION == 6 and _lib.GG_SCORE_MAX_LABELS == 64


def test_library_exports_and_binding_binds_the_score_symbols():
    build.build()
    L = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (gg_[a-z0-9_]+)", out))
    for s in SCORE_SYMBOLS:
        assert s in exported and s in _lib.SYMBOLS and getattr(L, s).argtypes is not None, s
    assert L.gg_abi_version() == 6
    # null contexts are refused before anything else is looked at
    ids = (C.c_int32 * 2)(40, 50)
    assert L.gg_set_score_labels(None, 2, ids) == -1
    assert L.gg_set_slot_scoring(None, 1, None, 0, 1) == -1
    assert L.gg_get_slot_scores(None, 1, None, 0, None) == -1
    assert L.gg_reset_slot_scores(None, 1, None, 0) == -1


def _device_rows(g, ids):
    """what gg_get_slot_scores would hold after the published run: per listed id (non-ground, ground), then the unlisted bin"""
    by_name = g["labels"]
    rows = []
    for lid in ids:
        row = by_name.get(LABELS[lid])
        rows.append((row["nonground"], row["total"] - row["nonground"]) if row else (0, 0))
    return rows + [(0, 0)]


def test_from_device_counts_reproduces_the_published_table():
    g = json.load(open(GOLDEN))
    ids = list(LABELS.keys())
    dev = GroundEvaluator.from_device_counts(ids, _device_rows(g, ids), clouds=g.get("clouds", 0))
    ref = GroundEvaluator.from_counts({k: v["nonground"] for k, v in g["labels"].items()}, {k: v["total"] for k, v in g["labels"].items()})
    ref.cloud_count = g.get("clouds", 0)
    assert dev.counters() == ref.counters()
    assert dev.table() == ref.table() and dev.rows() == ref.rows()
    s, S = dev.summary(), g["summary"]
    assert (s["TP"], s["FP"], s["FN"]) == (S["Precision"][1], S["Precision"][2], S["Recall"][2])
    for key, name in (("precision", "Precision"), ("recall", "Recall"), ("f1", "F1"), ("accuracy", "Accuracy"), ("iou_ground", "IoUg")):
        assert f"{s[key]:2.2%}" == f"{S[name][0]:.2f}%", key
    for name, row in g["labels"].items():
        assert dev.rows()["labels"][name]["nonground_pct"] == round(100.0 * row["nonground"] / row["total"], 2)
    # the caller's order of the ids is free
    perm = ids[::-1]
    assert GroundEvaluator.from_device_counts(perm, _device_rows(g, perm), clouds=g.get("clouds", 0)).counters() == ref.counters()


def test_from_device_counts_unknown_bin_raises_or_is_tolerated():
    ids = [40, 50, 70]
    rows = [(1, 5), (7, 2), (0, 3), (4, 6)]
    with pytest.raises(KeyError):
        GroundEvaluator.from_device_counts(ids, rows, clouds=2)
    ev = GroundEvaluator.from_device_counts(ids, rows, clouds=2, allow_unknown=True)
    assert (ev.unknown_non_ground, ev.unknown_total, ev.cloud_count) == (4, 10, 2)
    assert ev.total["road"] == 6 and ev.true_positive["road"] == 5 and ev.false_positive["building"] == 2 and ev.non_ground["building"] == 7
    GroundEvaluator.from_device_counts(ids, rows[:3] + [(0, 0)], clouds=2)          # an empty unknown bin is no error
    with pytest.raises(ValueError):
        GroundEvaluator.from_device_counts(ids, rows[:3])
    # ... and the same through add_cloud, the definition
    cpu = GroundEvaluator()
    with pytest.raises(KeyError):
        cpu.add_cloud(np.array([49, 99]), np.array([40, 7]))
    cpu = GroundEvaluator()
    cpu.add_cloud(np.array([49, 99, 99, 49]), np.array([40, 7, 65535, 7]), allow_unknown=True)
    assert (cpu.unknown_non_ground, cpu.unknown_total, cpu.total["road"]) == (2, 3, 1)


def test_add_cloud_points_applies_skip_nans_and_is_unchanged_without():
    sem = np.array([40, 40, 10, 10, 50, 72], dtype=np.uint16)
    pred = np.array([49, 99, 99, 49, 99, 49], dtype=np.uint8)
    xyz = np.array([[1, 1, 0], [1, 1, np.nan], [np.nan, 0, 0], [2, 2, 2], [0, np.nan, 1], [3, 3, np.inf]], dtype=np.float32)
    plain = GroundEvaluator()
    plain.add_cloud(pred, sem)
    assert plain.total["road"] == 2 and plain.total["car"] == 2 and plain.total["building"] == 1 and plain.cloud_count == 1
    none = GroundEvaluator()
    none.add_cloud(pred, sem, points=None)
    assert none.counters() == plain.counters()
    skipped = GroundEvaluator()
    skipped.add_cloud(pred, sem, points=xyz)
    assert skipped.total["road"] == 1 and skipped.non_ground["road"] == 0           # the NaN-z road point is gone
    assert skipped.total["car"] == 1 and skipped.false_positive["car"] == 1         # the NaN-x car point is gone
    assert skipped.total["building"] == 0 and skipped.total["terrain"] == 1         # NaN y gone, +inf stays
    assert skipped.cloud_count == 1
    structured = np.zeros(6, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ring", "<u2")])
    structured["x"], structured["y"], structured["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    again = GroundEvaluator()
    again.add_cloud(pred, sem, points=structured)
    assert again.counters() == skipped.counters()


def test_a_returned_point_never_has_a_nan_x_or_y_but_may_have_a_nan_z():
    """The device tests z alone for the skip_nans rule (k8_score.hip): held to the oracle on every hostile scene, every frame."""
    nan_z_returned = 0
    for sc in es.adversarial_scenes():
        ref = oracle.OracleMap(sc.length, sc.resolution, pos=sc.pos, odom_z=sc.odom_z)
        if sc.cfg_edit:
            sc.cfg_edit(ref.cfg)
        for frame in range(sc.frames):
            r = ref.filter_cloud(sc.cloud, tuple(float(v) for v in sc.origin), sc.base_z)
            out = r["out_points"]
            assert not np.isnan(out["x"]).any() and not np.isnan(out["y"]).any(), (sc.name, frame)
            emitted = r["index"] >= 0
            assert set(np.unique(r["label"][emitted])) <= {GROUND, NONGROUND} and not r["label"][~emitted].any(), (sc.name, frame)
            nan_z_returned += int(np.isnan(out["z"]).sum())
    assert nan_z_returned > 0  # NaN heights inside the map are returned: the rule is live
