"""gg_track_clusters without a GPU: the entry point is declared, exported, bound and reachable, the ctypes mirrors have the layout the C
compiler gives the two structs, and a null context is refused before the device is touched.  And the expectation of the GPU tests
(tests/tracks_ref.py) is held without the code under test: two independent formulations of the overlap matrix against each other, known
answers fixed by hand, and the invariants of the ids on random chains."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, build  # noqa: E402
from tests import tracks_ref  # noqa: E402

TRACK_FIELDS = ["track_id", "age", "prev", "overlap", "still", "cells", "sum_row", "sum_col"]
CALL_FIELDS = ["n", "d_cells", "cells_stride", "d_cells_prev", "prev_stride", "d_tracks_in", "d_heads_in", "shifts", "max_clusters", "gate", "order",
               "d_tracks_out", "d_heads_out", "d_cell_track", "track_stride"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- 1. the boundary

def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "groundgrid_hip.h")).read()
    assert re.search(r"^#define GG_HAS_TRACK_CLUSTERS 1$", header, re.M) and re.search(r"^#define GG_TRACK_MAX_CLUSTERS 1024$", header, re.M)
    assert re.search(r"^#define GG_ABI_VERSION 6$", header, re.M) or lib.gg_abi_version() == 6
    assert "gg_track_clusters" in _lib.SYMBOLS and _lib.GG_HAS_TRACK_CLUSTERS == 1 and _lib.GG_TRACK_MAX_CLUSTERS == 1024
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT gg_track_clusters\b", out)
    assert lib.gg_abi_version() == 6
    assert lib.gg_track_clusters(None, None, None) == -1  # a null context, before the device is touched
    x = _lib.GGClusterTracks()
    assert lib.gg_track_clusters(None, C.byref(x), None) == -1
    internal = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    assert f"TRACK_SLAB_WORDS = {_lib.GG_TRACK_SLAB_WORDS // 1024} * 1024" in internal


def test_struct_mirrors_match_the_header():
    assert [n for n, _ in _lib.GGTrack._fields_] == TRACK_FIELDS and [n for n, _ in _lib.GGClusterTracks._fields_] == CALL_FIELDS
    args = ["sizeof(gg_track)", "sizeof(gg_cluster_tracks)"] + [f"offsetof(gg_track, {m})" for m in TRACK_FIELDS] + [f"offsetof(gg_cluster_tracks, {m})" for m in CALL_FIELDS]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "groundgrid_hip.h"\nint main(void){ size_t v[] = {' + ", ".join(args) + \
           '}; for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]); printf("%d\\n", GG_TRACK_MAX_CLUSTERS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "t")], text=True).split()))
    want = [C.sizeof(_lib.GGTrack), C.sizeof(_lib.GGClusterTracks)] + [getattr(_lib.GGTrack, m).offset for m in TRACK_FIELDS] + \
           [getattr(_lib.GGClusterTracks, m).offset for m in CALL_FIELDS] + [_lib.GG_TRACK_MAX_CLUSTERS]
    assert vals == want and vals[0] == 32
    assert api.TRACK_DTYPE == tracks_ref.TRACK_DTYPE and api.TRACK_DTYPE.itemsize == 32 and list(api.TRACK_DTYPE.names) == TRACK_FIELDS


def test_python_method_has_the_documented_signature():
    sig = inspect.signature(api.GroundSegmentation.track_clusters)
    names = list(sig.parameters)
    assert names[:9] == ["self", "cell_cluster", "previous", "shifts", "max_clusters", "gate", "cell_track", "out", "on_torch_stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["previous"], d["shifts"], d["max_clusters"], d["gate"], d["cell_track"], d["out"], d["on_torch_stream"]) == (None, None, 256, 1, False, None, False)
    assert {"tracks", "heads", "cell_track", "cell_cluster"} <= set(api.TrackOutputs.__dataclass_fields__)


# ---------------------------------------------------------------- 2. two formulations of the overlap

def random_case(rng):
    side = int(rng.choice([23, 41]))
    g, M = int(rng.integers(0, 3)), int(rng.choice([4, 16, 256]))
    cur = tracks_ref.random_scene(rng, side, rng.choice([0.05, 0.2, 0.5]))
    prev = tracks_ref.random_scene(rng, side, rng.choice([0.05, 0.2, 0.5]))
    kind = rng.integers(0, 4)
    if kind == 0:
        shift = (0, 0)
    elif kind == 1:
        shift = tuple(int(v) for v in rng.integers(-3, 4, 2))
    elif kind == 2:
        shift = tuple(int(v) for v in rng.choice([-(side - 1), side - 1, -side, side, 0, 1], 2))
    else:
        shift = tuple(int(v) for v in rng.integers(-2 * side, 2 * side + 1, 2))
    tracks_in, heads_in = tracks_ref.first_records(prev, M, first_id=int(rng.integers(0, 1000)))
    return side, g, M, cur, prev, shift, tracks_in.view(tracks_ref.TRACK_DTYPE).reshape(-1), heads_in


def test_two_formulations_agree_on_random_cases():
    rng = np.random.default_rng(2301)
    nonzero = matrices = 0
    for _ in range(80):
        side, g, M, cur, prev, shift, tracks_in, heads_in = random_case(rng)
        Kc, Kp, _ = tracks_ref.cluster_counts(cur, prev, heads_in, M)
        a = tracks_ref.overlap_vectorised(cur, prev, Kc, Kp, M, shift, g)
        b = tracks_ref.overlap_loop(cur, prev, Kc, Kp, M, shift, g)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (side, g, M, shift)
        assert np.all(a[1] <= a[0])
        if abs(shift[0]) >= side or abs(shift[1]) >= side:
            assert not a[0].any()
        nonzero += bool(a[0].any())
        matrices += 1
        ra = tracks_ref.track_map(cur, prev, tracks_in, heads_in, shift, M, g, tracks_ref.overlap_vectorised)
        rb = tracks_ref.track_map(cur, prev, tracks_in, heads_in, shift, M, g, tracks_ref.overlap_loop)
        assert all(np.array_equal(u, v) for u, v in zip(ra, rb))
    assert matrices == 80 and nonzero >= 20


# ---------------------------------------------------------------- 3. known answers

BLOBS = {  # name: (rows, cols, (row, col) before, (drow, dcol))
    "3x4": (3, 4, (3, 3), (1, 0)),
    "2x2": (2, 2, (3, 15), (2, -2)),
    "5x1": (5, 1, (3, 27), (1, 1)),
    "1x1": (1, 1, (16, 4), (1, 1)),
    "4x4": (4, 4, (16, 16), (-1, 2)),
    "3x6": (3, 6, (28, 5), (0, -2)),
}


def blob_planes(side=41):
    before, after = np.zeros((side, side), bool), np.zeros((side, side), bool)
    for h, w, (r, q), (dr, dq) in BLOBS.values():
        before[r:r + h, q:q + w] = True
        after[r + dr:r + dr + h, q + dq:q + dq + w] = True
    return tracks_ref.label_plane(before), tracks_ref.label_plane(after)


def blob_id(plane, name, moved):
    h, w, (r, q), (dr, dq) = BLOBS[name]
    return int(plane[r + (dr if moved else 0), q + (dq if moved else 0)])


def test_known_answers_six_blobs():
    before, after = blob_planes()
    assert before.max() == after.max() == 5
    # the boxes are at least 2 g + 2 = 6 cells apart before and after, at g = 2
    for plane in (before, after):
        boxes = [(np.nonzero(plane == k)[0].min(), np.nonzero(plane == k)[0].max(), np.nonzero(plane == k)[1].min(), np.nonzero(plane == k)[1].max()) for k in range(6)]
        for i in range(6):
            for j in range(i + 1, 6):
                a, b = boxes[i], boxes[j]
                gap = max(a[0] - b[1], b[0] - a[1], a[2] - b[3], b[2] - a[3]) - 1
                assert gap >= 6
    M = 16
    tracks_in, heads_in = tracks_ref.first_records(before, M, first_id=100)
    tin = tracks_in.view(tracks_ref.TRACK_DTYPE).reshape(-1)
    # g = 2: every cluster inherits its predecessor's id
    rec, heads, plane = tracks_ref.track_map(after, before, tin, heads_in, (0, 0), M, 2)
    assert heads.tolist() == [106, 6, 0, 0]
    for name, (h, w, _, (dr, dq)) in BLOBS.items():
        c, p = blob_id(after, name, True), blob_id(before, name, False)
        assert rec[c]["prev"] == p and rec[c]["track_id"] == 100 + p and rec[c]["age"] == 1 and rec[c]["cells"] == h * w
        assert rec[c]["still"] == max(h - abs(dr), 0) * max(w - abs(dq), 0)
        # a rectangle against its moved self is separable: (pairs of rows within the gate) * (pairs of columns within the gate)
        along = lambda n, d: sum(1 for i in range(n) for j in range(n) if abs(j - (i + d)) <= 2)  # noqa: E731
        assert rec[c]["overlap"] == along(h, dr) * along(w, dq)
    assert np.array_equal(plane >= 0, after >= 0)


def test_known_answers_gate_zero_loses_the_three_that_left_their_cells():
    before, after = blob_planes()
    M = 16
    tracks_in, heads_in = tracks_ref.first_records(before, M, first_id=100)
    tin = tracks_in.view(tracks_ref.TRACK_DTYPE).reshape(-1)
    rec, heads, _ = tracks_ref.track_map(after, before, tin, heads_in, (0, 0), M, 0)
    assert heads.tolist() == [109, 6, 3, 3]
    lost = sorted(blob_id(after, name, True) for name in ("2x2", "5x1", "1x1"))
    assert [int(c) for c in np.nonzero(rec["prev"] < 0)[0]] == lost
    assert rec["track_id"][lost].tolist() == [106, 107, 108] and rec["age"][lost].tolist() == [0, 0, 0]
    for name in ("3x4", "4x4", "3x6"):
        h, w, _, (dr, dq) = BLOBS[name]
        c, p = blob_id(after, name, True), blob_id(before, name, False)
        assert rec[c]["prev"] == p and rec[c]["track_id"] == 100 + p
        assert rec[c]["overlap"] == rec[c]["still"] == (h - abs(dr)) * (w - abs(dq)) > 0
    # the same with the map moved under the scene: the shift takes the move out
    moved = np.full_like(after, -1)
    moved[2:, :-3] = after[:-2, 3:]  # the scan two rows down, three columns left: current (r, q) lies over previous (r - 2, q + 3)
    rec2, heads2, _ = tracks_ref.track_map(moved, before, tin, heads_in, (-2, 3), M, 0)
    assert heads2.tolist() == heads.tolist() and np.array_equal(rec2[["track_id", "age", "prev", "overlap", "still", "cells"]], rec[["track_id", "age", "prev", "overlap", "still", "cells"]])


def test_split_merge_and_ties():
    side, M = 23, 8
    prev = np.full((side, side), -1, np.int32)
    prev[5:7, 2:12] = 0  # one blob of 2 x 10
    tin, hin = tracks_ref.first_records(prev, M, first_id=7)
    tin = tin.view(tracks_ref.TRACK_DTYPE).reshape(-1)
    cur = np.full((side, side), -1, np.int32)
    cur[5:7, 2:5], cur[5:7, 6:12] = 0, 1  # a split into 3 and 6 columns: the larger part keeps the track
    rec, heads, _ = tracks_ref.track_map(cur, prev, tin, hin, (0, 0), M, 0)
    assert rec["track_id"].tolist() == [8, 7] and rec["prev"].tolist() == [-1, 0] and heads.tolist() == [9, 2, 1, 0]
    cur[:] = -1
    cur[5:7, 2:6], cur[5:7, 8:12] = 0, 1  # equal parts: the smaller c wins
    rec, heads, _ = tracks_ref.track_map(cur, prev, tin, hin, (0, 0), M, 0)
    assert rec["track_id"].tolist() == [7, 8] and rec["prev"].tolist() == [0, -1]
    # a merge: two previous blobs under one current; the larger overlap is continued, the other track ends; equal overlaps: the smaller p
    prev[:] = -1
    prev[5:7, 2:5], prev[5:7, 6:12] = 0, 1
    tin, hin = tracks_ref.first_records(prev, M, first_id=20)
    tin = tin.view(tracks_ref.TRACK_DTYPE).reshape(-1)
    cur[:] = -1
    cur[5:7, 2:12] = 0
    rec, heads, _ = tracks_ref.track_map(cur, prev, tin, hin, (0, 0), M, 0)
    assert rec["track_id"].tolist() == [21] and rec["overlap"].tolist() == [12] and heads.tolist() == [22, 1, 0, 1]
    prev[:] = -1
    prev[5:7, 2:6], prev[5:7, 8:12] = 0, 1
    rec, heads, _ = tracks_ref.track_map(cur, prev, tin, hin, (0, 0), M, 0)
    assert rec["track_id"].tolist() == [20] and rec["prev"].tolist() == [0] and heads.tolist() == [22, 1, 0, 1]


# ---------------------------------------------------------------- 4. invariants

def test_invariants_on_random_chains():
    rng = np.random.default_rng(2302)
    for case in range(40):
        side = int(rng.choice([23, 41]))
        M, g = int(rng.choice([4, 16, 256])), int(rng.integers(0, 3))
        cur = tracks_ref.random_scene(rng, side, 0.2)
        rec, heads, plane = tracks_ref.track_map(cur, M=M, g=g)
        assert rec["track_id"].tolist() == list(range(len(rec))) and heads.tolist() == [len(rec), len(rec), len(rec), 0] and not rec["age"].any()
        for frame in range(3):
            tin = np.zeros(M, tracks_ref.TRACK_DTYPE)
            tin[:len(rec)] = rec
            prev, hin = cur, heads
            keep = rng.random((side, side)) < 0.85
            cur = tracks_ref.label_plane(((prev >= 0) & keep) | (rng.random((side, side)) < 0.03))
            shift = (0, 0) if frame == 0 else tuple(int(v) for v in rng.integers(-2, 3, 2))
            if shift != (0, 0):
                cur = tracks_ref.label_plane(np.roll(cur >= 0, (-shift[0], -shift[1]), (0, 1)))
            rec, heads, plane = tracks_ref.track_map(cur, prev, tin, hin, shift, M, g)
            Kc, Kp, next_id = tracks_ref.cluster_counts(cur, prev, hin, M)
            assert len(rec) == Kc == heads[1]
            ids = rec["track_id"].tolist()
            assert len(set(ids)) == len(ids), "track ids are unique per map"
            inherited, new = rec[rec["prev"] >= 0], rec[rec["prev"] < 0]
            assert set(inherited["track_id"].tolist()) <= set(tin["track_id"][:Kp].tolist())
            assert len(set(inherited["prev"].tolist())) == len(inherited), "a predecessor is continued once"
            assert new["track_id"].tolist() == list(range(next_id, next_id + len(new))) and heads[2] == len(new)
            assert heads[3] + len(inherited) == Kp and heads[0] == next_id + len(new)
            assert np.all(inherited["age"] == tin["age"][inherited["prev"]] + 1) and not new["age"].any()
            assert np.all(inherited["overlap"] >= inherited["still"]) and np.all(inherited["overlap"] > 0)
            assert rec["cells"].sum() == ((cur >= 0) & (cur < M)).sum()
            assert np.array_equal(plane >= 0, (cur >= 0) & (cur < M))


def test_ids_wrap_at_31_bits_and_ages_saturate():
    side, M = 23, 4
    prev = np.full((side, side), -1, np.int32)
    prev[3, 3] = 0
    tin = np.zeros(M, tracks_ref.TRACK_DTYPE)
    tin[0] = (5, 2 ** 31 - 1, -1, 0, 0, 1, 3, 3)
    cur = np.full((side, side), -1, np.int32)
    cur[3, 3], cur[10, 10], cur[20, 20] = 0, 1, 2
    rec, heads, _ = tracks_ref.track_map(cur, prev, tin, [2 ** 31 - 1, 1, 0, 0], (0, 0), M, 0)
    assert rec["track_id"].tolist() == [5, 2 ** 31 - 1, 0] and rec["age"].tolist() == [2 ** 31 - 1, 0, 0] and heads.tolist() == [1, 3, 2, 0]


# ---------------------------------------------------------------- 5. the host helper

def test_motion_takes_the_shift_out():
    import torch

    before, after = blob_planes()
    M = 16
    tin, hin = tracks_ref.first_records(before, M)
    moved = np.full_like(after, -1)
    moved[2:, :-3] = after[:-2, 3:]
    rec, heads, _ = tracks_ref.track_map(moved, before, tin.view(tracks_ref.TRACK_DTYPE).reshape(-1), hin, (-2, 3), M, 2)
    full = np.zeros(M, tracks_ref.TRACK_DTYPE)
    full[:len(rec)] = rec
    old = api.TrackOutputs(tracks=torch.from_numpy(tin.copy())[None], heads=torch.from_numpy(hin.copy())[None])
    new = api.TrackOutputs(tracks=torch.from_numpy(full.view(np.int32).reshape(M, 8).copy())[None], heads=torch.from_numpy(heads.copy())[None])
    motion = new.motion(old, shifts=[[-2, 3]], resolution=0.5)
    assert motion.shape == (1, M, 2) and motion.dtype == np.float64 and np.isnan(motion[0, 6:]).all()
    for name, (_, _, _, (dr, dq)) in BLOBS.items():
        c = blob_id(after, name, True)  # (`moved` keeps the ids of `after`)
        assert motion[0, c].tolist() == [-0.5 * dr, -0.5 * dq], name
    assert new.table(0).tolist() == rec.tolist()
