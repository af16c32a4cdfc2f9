"""gg_fuse_states without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version and the neighbouring structs are what they were, a null context is refused before
the device is touched, and the Python entry point refuses bad arguments before any library call.  And the expectation of the GPU tests
(tests/fusion_ref.py) is held without the code under test: against a world-anchored array that is never shifted (the one check of the
sign of the shift that does not share the definition's arithmetic), and on a few facts fixed by hand."""
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
from tests import fusion_ref  # noqa: E402

FIELDS = ["n", "d_state", "state_stride", "d_evidence_in", "shifts", "hit", "miss", "decay", "e_min", "e_max", "free_threshold", "occ_threshold",
          "order", "d_evidence_out", "plane_stride", "d_fused", "d_frontier", "d_counts"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def compile_and_run(prog):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
        return subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, check=True).stdout.decode()


# ---------------------------------------------------------------- the ABI

def test_symbol_is_exported_and_bound(lib):
    assert "gg_fuse_states" in _lib.SYMBOLS
    assert hasattr(lib, "gg_fuse_states")
    assert len(lib.gg_fuse_states.argtypes) == 3


def test_struct_layout_equals_the_ctypes_mirror(lib):
    assert [f[0] for f in _lib.GGStateFusion._fields_] == FIELDS
    lines = ['printf("%zu\\n", sizeof(gg_state_fusion));'] + [f'printf("%zu\\n", offsetof(gg_state_fusion, {k}));' for k in FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    assert [int(v) for v in out.split()] == [C.sizeof(_lib.GGStateFusion)] + [getattr(_lib.GGStateFusion, k).offset for k in FIELDS]


def test_feature_macro_is_defined(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_FUSE_STATES) || GG_HAS_FUSE_STATES != 1
    #error "GG_HAS_FUSE_STATES"
    #endif
    int main(void) { printf("%d %d %d %d\n", GG_HAS_FUSE_STATES, GG_CELL_FREE, GG_CELL_UNKNOWN, GG_CELL_OCCUPIED); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, fusion_ref.FREE, fusion_ref.UNKNOWN, fusion_ref.OCCUPIED]


def test_abi_version_and_the_other_structs_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu %zu %zu %zu %zu %zu\n", GG_ABI_VERSION, sizeof(gg_batch), sizeof(gg_cloud_raster), sizeof(gg_cloud_split), sizeof(gg_cloud_clusters),
                            sizeof(gg_cloud_clearance), sizeof(gg_cloud_visibility)); return 0; }
    ''')
    version, batch, raster, split, clusters, clearance, visibility = (int(v) for v in out.split())
    assert version == 6
    assert batch == C.sizeof(_lib.GGBatch) == 120
    assert raster == C.sizeof(_lib.GGCloudRaster) == 96
    assert split == C.sizeof(_lib.GGCloudSplit) == 128
    assert clusters == C.sizeof(_lib.GGCloudClusters) == 144
    assert clearance == C.sizeof(_lib.GGCloudClearance) == 152
    assert visibility == C.sizeof(_lib.GGCloudVisibility) == 128


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int frame(gg_context *ctx, const int32_t *d_state, const int32_t *d_before, int32_t *d_after, int32_t *d_fused, int32_t *d_frontier, int32_t *d_counts,
              const int32_t *shifts, void *stream) {
        gg_state_fusion x = {0};
        x.n = 2;
        x.d_state = d_state;
        x.state_stride = 364 * 364;
        x.d_evidence_in = d_before;
        x.shifts = shifts;
        x.hit = 4;  x.miss = 1;  x.decay = 0;
        x.e_min = -16;  x.e_max = 32;
        x.free_threshold = -2;  x.occ_threshold = 4;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_evidence_out = d_after;
        x.plane_stride = 364 * 364;
        x.d_fused = d_fused;
        x.d_frontier = d_frontier;
        x.d_counts = d_counts;
        return gg_fuse_states(ctx, &x, stream);
    }
    int main(void) { return frame(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGStateFusion()
    x.n = 1
    assert lib.gg_fuse_states(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_fuse_states(None, None, None) == -1
    x.n = 0
    assert lib.gg_fuse_states(None, C.byref(x), None) == -1


def test_the_mirrored_tile_is_the_kernels():
    text = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    tile = tuple(int(re.search(rf"constexpr int FUSE_TILE_{k} = (\d+);", text).group(1)) for k in "XY")
    assert tile == _lib.GG_FUSE_TILE
    assert _lib.GG_FUSE_LIMIT == fusion_ref.LIMIT == 2 ** 30 - 1


# ---------------------------------------------------------------- the Python entry point

def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.fuse_states).parameters
    assert list(params)[:3] == ["self", "states", "evidence"]
    assert params["evidence"].default is None
    defaults = {"shifts": None, **fusion_ref.DEFAULTS, "order": "row", "fused": True, "frontier": True, "counts": True, "out": None, "on_torch_stream": False}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.FusionOutputs.__dataclass_fields__] == ["evidence", "state", "frontier", "counts"]


class NoLibrary:
    """in place of the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def test_python_entry_point_refuses_bad_arguments_before_any_library_call(lib):
    import torch

    seg = api.GroundSegmentation()
    seg._L, seg.rows, seg.cols, seg.device, seg.n_slots = NoLibrary(), 20, 20, 0, 4
    host = torch.zeros((2, 20, 20), dtype=torch.int32)
    with pytest.raises(ValueError):  # (not on the device)
        seg.fuse_states(host)
    for bad in (None, np.zeros((2, 20, 20), np.int32), "planes"):
        with pytest.raises(ValueError):
            seg.fuse_states(bad)
    lim = fusion_ref.LIMIT
    for kw in (dict(order="fortran"), dict(hit=-1), dict(miss=-1), dict(decay=-1), dict(hit=lim + 1), dict(miss=lim + 1), dict(decay=lim + 1), dict(hit=1.5),
               dict(decay=True), dict(e_min=1), dict(e_max=-1), dict(e_min=-lim - 1), dict(e_max=lim + 1), dict(free_threshold=0), dict(free_threshold=-17),
               dict(occ_threshold=0), dict(occ_threshold=33), dict(e_min=0), dict(e_max=0), dict(e_max=None)):
        with pytest.raises(ValueError, match=r"fuse_states: (?!states must)"):  # (the parameter is named, not the planes)
            seg.fuse_states(host, **kw)


# ---------------------------------------------------------------- the reference, without the code under test

SIDE = 20
DRIVE_SHIFTS = [(0, 0), (1, -1), (-1, 1), (3, 2), (-(SIDE - 1), 0), (SIDE - 1, 0), (0, SIDE - 1), (2, -(SIDE - 1)), (-2, -3), (0, -SIDE), (SIDE, 1),
                (-1, 0), (1, 1), (-3 * SIDE, 5), (0, 1), (4, 2 * SIDE + 3), (-2, -1)]


def random_states(rng, rows, cols):
    """observations in {-1, 0, 1} and a few other positive and negative words"""
    s = rng.integers(-1, 2, (rows, cols)).astype(np.int32)
    odd = rng.random((rows, cols)) < 0.05
    s[odd] = rng.choice(np.array([2, 7, -2, -9, 2 ** 31 - 1, -2 ** 31], np.int64), int(odd.sum())).astype(np.int32)
    return s


def drive(shifts, p, seed, flip=1):
    """the chained definition against the world-anchored array; returns the number of compared cells that differ and that were compared"""
    rng = np.random.default_rng(seed)
    world = fusion_ref.WorldEvidence(SIDE, SIDE, shifts, p)
    evidence, differ, compared = None, 0, 0
    for shift in shifts:
        state = random_states(rng, SIDE, SIDE)
        evidence = fusion_ref.expected_fusion(state, evidence, (flip * shift[0], flip * shift[1]), p)["evidence"]
        world.step(shift, state)
        ok = world.comparable()
        differ += int((evidence[ok] != world.evidence()[ok]).sum())
        compared += int(ok.sum())
    return differ, compared


@pytest.mark.parametrize("p", [fusion_ref.params(), fusion_ref.params(decay=1, hit=3, miss=2, e_min=-7, e_max=9, free_threshold=-7, occ_threshold=9)])
def test_the_definition_equals_a_world_anchored_array(p):
    assert len(DRIVE_SHIFTS) >= 12
    mags = {abs(v) for s in DRIVE_SHIFTS for v in s}
    assert {0, 1, SIDE - 1, SIDE}.issubset(mags) and max(mags) > SIDE and {(-1) ** k * m for m in (1, SIDE - 1, SIDE) for k in (0, 1)} <= {v for s in DRIVE_SHIFTS for v in s}
    differ, compared = drive(DRIVE_SHIFTS, p, 7300)
    assert differ == 0 and compared > 8 * SIDE * SIDE
    # the check has teeth: with the sign of the shift turned round the two part ways
    differ, _ = drive(DRIVE_SHIFTS, p, 7300, flip=-1)
    assert differ > SIDE * SIDE


def test_a_random_walk_equals_the_world_anchored_array():
    rng = np.random.default_rng(7301)
    shifts = [tuple(int(v) for v in rng.integers(-4, 5, 2)) for _ in range(12)]
    differ, compared = drive(shifts, fusion_ref.params(decay=1), 7302)
    assert differ == 0 and compared >= 12 * SIDE * SIDE // 2


# ---------------------------------------------------------------- fixed facts of the expectation

def test_one_hit_marks_and_misses_clear_under_the_defaults():
    p = fusion_ref.params()
    state = np.zeros((5, 5), np.int32)
    state[2, 2] = 1
    state[0, :] = -1
    first = fusion_ref.expected_fusion(state, None, None, p)
    assert first["evidence"][2, 2] == 4 and first["fused"][2, 2] == fusion_ref.OCCUPIED
    assert (first["evidence"][0] == -1).all() and (first["fused"][0] == fusion_ref.UNKNOWN).all()  # one miss does not free a cell
    assert (first["frontier"] == -1).all() and first["counts"].tolist() == [0, 24, 1, 0]
    second = fusion_ref.expected_fusion(-np.ones((5, 5), np.int32), first["evidence"], None, p)
    assert (second["fused"][0] == fusion_ref.FREE).all() and second["fused"][2, 2] == fusion_ref.UNKNOWN and second["evidence"][2, 2] == 3
    assert second["frontier"][0].tolist() == [0] * 5 and (second["frontier"][1:] == -1).all()
    assert second["counts"].tolist() == [5, 20, 0, 5]


def test_the_shift_brings_the_cell_the_map_scrolled_to():
    """gg_move_maps: new(r, c) = old(r + s0, c + s1).  Evidence at (4, 1) before a shift of (2, -1) lies at (2, 2) after it"""
    p = fusion_ref.params()
    before = np.zeros((6, 6), np.int32)
    before[4, 1] = 9
    before[0, 0] = 100   # clamped to e_max, then out of the window
    before[5, 0] = -100  # clamped to e_min on the way
    after = fusion_ref.expected_fusion(np.zeros((6, 6), np.int32), before, (2, -1), p)["evidence"]
    assert after[2, 2] == 9 and after[3, 1] == -16 and int(np.abs(after).sum()) == 25
    for shift in ((6, 0), (0, -6), (-40, 3), (2 ** 31 - 1, 0), (0, -2 ** 31)):
        assert not fusion_ref.expected_fusion(np.zeros((6, 6), np.int32), before, shift, p)["evidence"].any()


def test_decay_stops_at_zero_and_the_border_has_no_neighbours_beyond_it():
    p = fusion_ref.params(decay=5, hit=0, miss=0)
    before = np.array([[3, -3, 7, -7]], np.int32)
    assert fusion_ref.expected_fusion(np.zeros((1, 4), np.int32), before, None, p)["evidence"].tolist() == [[0, 0, 2, -2]]
    free = -np.ones((3, 3), np.int32)
    got = fusion_ref.expected_fusion(free, free * 8, None, fusion_ref.params())
    assert (got["fused"] == fusion_ref.FREE).all() and (got["frontier"] == -1).all()  # free to the border: no frontier
    free[0, 0] = 0
    got = fusion_ref.expected_fusion(free, None, None, fusion_ref.params(miss=2))
    assert got["fused"][0, 0] == fusion_ref.UNKNOWN and sorted(map(tuple, np.argwhere(got["frontier"] == 0))) == [(0, 1), (1, 0), (1, 1)]
