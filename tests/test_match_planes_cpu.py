"""gg_match_planes without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version is what it was, a null context is refused before the device is touched, and the
Python entry point refuses bad arguments before any library call.  And the expectation of the GPU tests (tests/match_ref.py: one candidate
at a time by one integer gather, the best by a lexicographic sort) is held without the code under test: against a restatement that shares
no code with it (per yaw the count plane of the rotated cells by np.add.at on a padded canvas, correlated by scipy with the clamped,
zero-padded field, the best by a scan in rank order), and on closed forms and facts fixed by hand."""
import ctypes as C
import inspect
import math
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
from tests import fusion_ref, match_ref  # noqa: E402

UNIT = match_ref.UNIT
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
FIELDS = ["n", "d_scan", "scan_stride", "d_field", "field_stride", "field_max", "shifts", "pivots", "rotations", "n_rotations", "window", "order",
          "d_best", "d_scores", "score_stride"]


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
    assert "gg_match_planes" in _lib.SYMBOLS
    assert hasattr(lib, "gg_match_planes")
    assert len(lib.gg_match_planes.argtypes) == 3


def test_struct_layout_equals_the_ctypes_mirror(lib):
    assert [f[0] for f in _lib.GGPlaneMatches._fields_] == FIELDS
    lines = ['printf("%zu\\n", sizeof(gg_plane_matches));'] + [f'printf("%zu\\n", offsetof(gg_plane_matches, {k}));' for k in FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    assert [int(v) for v in out.split()] == [C.sizeof(_lib.GGPlaneMatches)] + [getattr(_lib.GGPlaneMatches, k).offset for k in FIELDS]


def test_feature_macro_and_the_limits_are_defined(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_MATCH_PLANES) || GG_HAS_MATCH_PLANES != 1
    #error "GG_HAS_MATCH_PLANES"
    #endif
    int main(void) { printf("%d %d %d %d %d\n", GG_HAS_MATCH_PLANES, GG_MATCH_MAX_WINDOW, GG_MATCH_MAX_ROTATIONS, GG_MATCH_UNIT, GG_ABI_VERSION); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, 32, 64, 16384, 6]
    assert (_lib.GG_HAS_MATCH_PLANES, _lib.GG_MATCH_MAX_WINDOW, _lib.GG_MATCH_MAX_ROTATIONS, _lib.GG_MATCH_UNIT) == (1, 32, 64, 16384)
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int match(gg_context *ctx, const int32_t *d_state, const int32_t *d_evidence, const int32_t *shifts, const int32_t *pivots, const int32_t *table,
              int32_t *d_best, int32_t *d_scores, void *stream) {
        gg_plane_matches x = {0};
        x.n = 2;
        x.d_scan = d_state;  x.scan_stride = 364 * 364;
        x.d_field = d_evidence;  x.field_stride = 364 * 364;  x.field_max = 32;
        x.shifts = shifts;  x.pivots = pivots;  x.rotations = table;  x.n_rotations = 21;
        x.window = 8;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_best = d_best;
        x.d_scores = d_scores;  x.score_stride = 21 * 17 * 17;
        return gg_match_planes(ctx, &x, stream);
    }
    int main(void) { return match(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGPlaneMatches()
    x.n = 1
    assert lib.gg_match_planes(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_match_planes(None, None, None) == -1
    x.n = 0
    assert lib.gg_match_planes(None, C.byref(x), None) == -1


def test_the_mirrored_constants_are_the_kernels():
    internal = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    kernel = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "k20_match.hip")).read()
    assert int(re.search(r"constexpr int MATCH_MAX_WINDOW = (\d+);", internal).group(1)) == _lib.GG_MATCH_MAX_WINDOW == match_ref.MAX_WINDOW
    assert int(re.search(r"constexpr int MATCH_MAX_ROTATIONS = (\d+);", internal).group(1)) == _lib.GG_MATCH_MAX_ROTATIONS == match_ref.MAX_ROTATIONS
    assert int(re.search(r"constexpr int MATCH_CHUNK = (\d+);", kernel).group(1)) == _lib.GG_MATCH_CHUNK
    assert int(re.search(r"constexpr int MATCH_LIST = (\d+);", kernel).group(1)) == _lib.GG_MATCH_LIST
    assert _lib.GG_MATCH_LIMIT == match_ref.LIMIT == 2 ** 31 - 1 and _lib.GG_MATCH_MAX_SIDE == match_ref.MAX_SIDE == 32768
    assert _lib.GG_MATCH_UNIT == UNIT


# ---------------------------------------------------------------- the Python entry point

def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.match_planes).parameters
    assert list(params)[:3] == ["self", "scan", "field"]
    defaults = {"shifts": None, "pivots": None, "rotations": None, **match_ref.DEFAULTS, "order": "row", "scores": False, "out": None, "on_torch_stream": False}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.MatchOutputs.__dataclass_fields__] == ["best", "scores"]
    assert match_ref.DEFAULTS["field_max"] == fusion_ref.DEFAULTS["e_max"]  # (an evidence plane of the defaults is read unclamped)


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
        seg.match_planes(host, host)
    for bad in (None, np.zeros((2, 20, 20), np.int32), "planes"):
        with pytest.raises(ValueError):
            seg.match_planes(bad, host)
    for kw in (dict(order="fortran"), dict(window=-1), dict(window=33), dict(window=True), dict(window=2.0), dict(window=None), dict(field_max=0), dict(field_max=-3),
               dict(field_max=1.5), dict(field_max=(2 ** 31 - 1) // 400 + 1), dict(rotations=[]), dict(rotations=[[UNIT, 0]] * 65), dict(rotations=[UNIT, 0, 1]),
               dict(rotations=[[UNIT + 1, 0]]), dict(rotations=[[0, -UNIT - 1]]), dict(rotations=[[0.5, 0]]), dict(rotations="table"), dict(rotations=[[2 ** 40, 0]])):
        with pytest.raises(ValueError, match=r"match_planes: (?!scan must)"):  # (the parameter is named, not the planes)
            seg.match_planes(host, host, **kw)
    seg.rows = 32769
    with pytest.raises(ValueError, match="rows or columns"):
        seg.match_planes(host, host, field_max=1)


def test_rotation_table():
    deg = [0.0, 90.0, -90.0, 180.0, 30.0, 0.2]
    want = [[16384, 0], [0, 16384], [0, -16384], [-16384, 0], [14189, 8192], [16384, 57]]
    for table in (api.rotation_table(np.radians(deg)), match_ref.rotation_table(np.radians(deg))):
        assert table.dtype == np.int32 and table.tolist() == want
    assert api.rotation_table(0.0).tolist() == [[16384, 0]] and api.rotation_table([]).shape == (0, 2)
    # half away from zero in both signs: 16384 cos(x) = 8191.5 is no float64 value of cos, so the rule is pinned on the rounding function
    fine = np.radians(np.linspace(-180.0, 180.0, 7201))
    assert np.array_equal(api.rotation_table(fine), match_ref.rotation_table(fine))
    assert np.abs(api.rotation_table(fine)).max() == UNIT
    for bad in ([np.nan], [[0.0, 1.0]], [np.inf]):
        with pytest.raises(ValueError):
            api.rotation_table(bad)


# ---------------------------------------------------------------- the reference against a restatement that shares no code with it

def correlated(scan, field, shift, pivot, rotations, W, field_max):
    """per yaw: the count plane of the rotated, shifted cells on a canvas that holds them all, correlated with the clamped field laid into the
    same canvas; the best by a walk in rank order that keeps the first strict improvement"""
    from scipy.signal import correlate2d

    rows, cols = scan.shape
    s0, s1 = int(np.clip(shift[0], -rows, rows)), int(np.clip(shift[1], -cols, cols))
    pad = 3 * max(rows, cols) + 2  # |rotated offset| <= 2 * side, |shift| <= side
    canvas = (rows + 2 * pad, cols + 2 * pad)
    reward = np.zeros((canvas[0] + 2 * W, canvas[1] + 2 * W), np.int64)
    reward[W + pad: W + pad + rows, W + pad: W + pad + cols] = np.minimum(np.maximum(field.astype(np.int64), 0), field_max)
    cells = [(r, c) for r in range(rows) for c in range(cols) if scan[r, c] > 0]
    volume = []
    for cq, sq in rotations.tolist():
        count = np.zeros(canvas, np.int64)
        where = []
        for r, c in cells:
            a, b = cq * (r - pivot[0]) - sq * (c - pivot[1]), sq * (r - pivot[0]) + cq * (c - pivot[1])
            ra = int(math.copysign((abs(a) + 8192) // 16384, a)) if a else 0
            rb = int(math.copysign((abs(b) + 8192) // 16384, b)) if b else 0
            where.append((pad + pivot[0] + ra + s0, pad + pivot[1] + rb + s1))
        if where:
            np.add.at(count, tuple(np.array(where).T), 1)
        volume.append(correlate2d(reward, count, mode="valid"))
    volume = np.stack(volume)
    assert volume.shape == (len(rotations), 2 * W + 1, 2 * W + 1)
    ranked = sorted((dy * dy + dx * dx, k, dy, dx) for k in range(len(rotations)) for dy in range(-W, W + 1) for dx in range(-W, W + 1))
    best, top = None, -1
    for _, k, dy, dx in ranked:
        if volume[k, dy + W, dx + W] > top:
            best, top = (k, dy, dx), int(volume[k, dy + W, dx + W])
    return np.array(list(best) + [top, len(cells), int((volume == top).sum())], np.int32), volume.astype(np.int32)


@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("rows,cols", [(9, 13), (20, 20)])
def test_reference_equals_the_correlation(rows, cols, order):
    """seeded random planes; `order` only changes how a plane would lie in memory, so the logical result is the same and lay() is an involution"""
    rng = np.random.default_rng(100 * rows + cols)
    table = np.array([[UNIT, 0], [14189, 8192], [0, -UNIT], [12000, -9000], [-UNIT, UNIT]], np.int32)
    for trial in range(6):
        scan = np.where(rng.random((rows, cols)) < 0.2, rng.integers(1, 5, (rows, cols)), rng.integers(-3, 1, (rows, cols))).astype(np.int32)
        field = rng.integers(-10, 30, (rows, cols)).astype(np.int32)
        shift = (int(rng.integers(-rows - 3, rows + 4)), int(rng.integers(-4, 5))) if trial % 3 == 0 else (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        pivot = (int(rng.integers(0, rows)), int(rng.integers(0, cols)))
        W, field_max = int(rng.integers(0, 5)), int(rng.integers(1, 25))
        want = match_ref.expected_match(scan, field, shift=shift, pivot=pivot, rotations=table, window=W, field_max=field_max)
        best, volume = correlated(scan, field, shift, pivot, table, W, field_max)
        assert np.array_equal(want["scores"], volume), trial
        assert want["best"].tolist() == best.tolist(), trial
        laid = match_ref.lay(scan, order)
        assert laid.shape == ((rows, cols) if order == "row" else (cols, rows)) and np.array_equal(match_ref.lay(laid, order), scan)
    plain = match_ref.expected_match(scan, field, window=2, field_max=9)  # the defaults: no shift, the centre, the identity
    best, volume = correlated(scan, field, (0, 0), (rows // 2, cols // 2), match_ref.IDENTITY, 2, 9)
    assert np.array_equal(plain["scores"], volume) and plain["best"].tolist() == best.tolist()


# ---------------------------------------------------------------- closed forms

@pytest.mark.parametrize("order", ["row", "col"])
def test_a_displaced_scan_is_found_with_the_sign_of_the_header(order):
    """the scan is the field's positive set displaced by (a, b): scan cell (r + a, c + b) for field cell (r, c).  Scan cell (R, C) then lies
    over field cell (R - a, C - b): the answer is (0, -a, -b), in (row, col) terms whatever the order of the planes in memory"""
    rng = np.random.default_rng(7)
    rows, cols, W = 24, 31, 5
    inner = np.zeros((rows, cols), bool)
    inner[W + 1: rows - W - 1, W + 1: cols - W - 1] = rng.random((rows - 2 * W - 2, cols - 2 * W - 2)) < 0.15
    field = np.where(inner, 20, -4).astype(np.int32)
    for a, b in ((0, 0), (3, -2), (-5, 5), (W, 0), (0, -W), (-1, -4)):
        scan = np.zeros((rows, cols), np.int32)
        r, c = np.nonzero(inner)
        scan[r + a, c + b] = 1
        # the planes pass through memory order and back, as a caller's would
        got = match_ref.expected_match(match_ref.lay(match_ref.lay(scan, order), order), match_ref.lay(match_ref.lay(field, order), order), window=W, field_max=32)
        assert got["best"].tolist() == [0, -a, -b, 20 * int(inner.sum()), int(inner.sum()), 1], (a, b)
        # with the displacement as the prior shift nothing is left to correct
        assert match_ref.expected_match(scan, field, shift=(-a, -b), window=W, field_max=32)["best"][:4].tolist() == [0, 0, 0, 20 * int(inner.sum())]


def test_quarter_turn_and_rounding():
    scan = np.zeros((9, 9), np.int32)
    cells = [(1, 2), (4, 4), (7, 3), (0, 8), (8, 0)]
    for r, c in cells:
        scan[r, c] = 1
    pivot = (4, 5)
    rr, cc = match_ref.rotated_cells(scan, pivot, (0, UNIT))  # (dr, dc) -> (-dc, dr), exactly
    assert sorted(zip(rr.tolist(), cc.tolist())) == sorted((pivot[0] - (c - pivot[1]), pivot[1] + (r - pivot[0])) for r, c in cells)
    rr, cc = match_ref.rotated_cells(scan, pivot, (UNIT, 0))
    assert sorted(zip(rr.tolist(), cc.tolist())) == sorted(cells)
    rr, cc = match_ref.rotated_cells(scan, pivot, (-UNIT, 0))  # the half turn
    assert sorted(zip(rr.tolist(), cc.tolist())) == sorted((2 * pivot[0] - r, 2 * pivot[1] - c) for r, c in cells)
    # one half, (8192, 0), on dr = +1 and -1: a = +-8192 rounds to +-1, away from zero in both signs; 8191 rounds to 0
    pair = np.zeros((9, 9), np.int32)
    pair[5, 5] = pair[3, 5] = 1
    rr, cc = match_ref.rotated_cells(pair, pivot, (8192, 0))
    assert sorted(zip(rr.tolist(), cc.tolist())) == [(3, 5), (5, 5)]
    rr, cc = match_ref.rotated_cells(pair, pivot, (8191, 0))
    assert sorted(zip(rr.tolist(), cc.tolist())) == [(4, 5), (4, 5)]  # (both land on the pivot, and both count)
    assert match_ref.rnd([8192, -8192, 8191, -8191, 24576, -24576, 0]).tolist() == [1, -1, 0, 0, 2, -2, 0]
    field = np.zeros((9, 9), np.int32)
    field[4, 5] = 7
    assert match_ref.expected_match(pair, field, pivot=pivot, rotations=[[8191, 0]], window=0, field_max=9)["best"].tolist() == [0, 0, 0, 14, 2, 1]


def test_everything_outside_scores_zero_and_the_tie_rule_decides():
    rng = np.random.default_rng(3)
    rows, cols, W = 12, 15, 3
    scan = (rng.random((rows, cols)) < 0.3).astype(np.int32)
    scan[5:8, 6:9] = 1
    field = rng.integers(1, 9, (rows, cols)).astype(np.int32)
    table = np.array([[UNIT, 0], [0, UNIT]], np.int32)
    # only cells near the pivot: a shift of a whole side leaves every window outside
    near = np.zeros_like(scan)
    near[5:8, 6:9] = 1
    for shift in ((rows, 0), (-rows - 50, 2), (0, cols), (1, -cols - 1), (I32_MAX, I32_MIN)):
        got = match_ref.expected_match(near, field, shift=shift, rotations=table, window=W, field_max=9)
        assert not got["scores"].any()
        assert got["best"].tolist() == [0, 0, 0, 0, 9, 2 * (2 * W + 1) ** 2], shift
    # rim cells come back inside under a window: the clamped shift is a side, not more
    assert match_ref.expected_match(scan, field, shift=(rows + 50, 0), window=W, field_max=9)["scores"].any() == bool(scan[:W].any())
    empty = match_ref.expected_match(np.zeros_like(scan), field, rotations=table, window=W, field_max=9)
    assert empty["best"].tolist() == [0, 0, 0, 0, 0, 2 * (2 * W + 1) ** 2]


def test_field_words_beyond_the_clamps_and_the_limit_at_its_edge():
    rows, cols = 6, 7
    scan = np.ones((rows, cols), np.int32)
    field = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, 11, 12, 13, I32_MAX - 1, I32_MAX], np.int64)
    field = np.resize(field, rows * cols).reshape(rows, cols).astype(np.int32)
    got = match_ref.expected_match(scan, field, window=0, field_max=12)
    assert got["best"][3] == int(np.clip(field.astype(np.int64), 0, 12).sum()) and got["best"][4] == rows * cols
    top = (2 ** 31 - 1) // (rows * cols)
    assert match_ref.accepts(top, rows, cols) and not match_ref.accepts(top + 1, rows, cols) and not match_ref.accepts(0, rows, cols)
    full = match_ref.expected_match(scan, np.full((rows, cols), I32_MAX, np.int32), window=1, field_max=top)
    assert full["best"].tolist() == [0, 0, 0, top * rows * cols, rows * cols, 1] and top * rows * cols > 2 ** 31 - 1 - rows * cols
    with pytest.raises(AssertionError):
        match_ref.expected_match(scan, field, window=0, field_max=top + 1)
    assert match_ref.accepts(1, 32768, 32768) and match_ref.accepts(1, 46340, 46340) and not match_ref.accepts(2, 32768, 32768)


def test_a_symmetric_scene_exercises_every_level_of_the_tie_rule():
    m, W = 6, 2
    scan = np.zeros((13, 13), np.int32)
    scan[m, m] = 1  # on the pivot: every rotation keeps it
    table = np.array([[UNIT, 0], [0, UNIT], [-UNIT, 0]], np.int32)

    def best(cells, **kw):
        field = np.full((13, 13), -1, np.int32)
        for (dy, dx), v in cells.items():
            field[m + dy, m + dx] = v
        return match_ref.expected_match(scan, field, rotations=table, window=W, field_max=9, **kw)["best"].tolist()

    assert best({(2, 2): 5, (0, 1): 4}) == [0, 2, 2, 5, 1, 3]                          # the score before the distance
    assert best({(2, 2): 5, (0, 1): 5, (-2, 0): 5}) == [0, 0, 1, 5, 1, 9]              # the smallest dy^2 + dx^2
    assert best({(1, 0): 5, (-1, 0): 5, (0, 1): 5, (0, -1): 5}) == [0, -1, 0, 5, 1, 12]  # ... then k = 0, then the smallest dy
    assert best({(0, 1): 5, (0, -1): 5}) == [0, 0, -1, 5, 1, 6]                         # ... then the smallest dx
    # k decides only after the distance: a second cell off the pivot makes the quarter turn the one yaw that reaches (0, 0), the identity (1, -1)
    scan[m, m + 1] = 1
    two = {(0, 0): 5, (-1, 0): 5}  # the quarter turn carries (0, +1) to (-1, 0)
    assert best(two) == [1, 0, 0, 10, 2, 1]
    # the identity and the quarter turn both reach 10 at (0, 0): the smaller k; the half turn, cells (0, 0) and (0, -1), reaches it at (0, +1)
    two = {(0, 0): 5, (-1, 0): 5, (0, 1): 5}
    assert best(two) == [0, 0, 0, 10, 2, 3]


def test_rotation_defaults_and_non_unit_pairs():
    rng = np.random.default_rng(11)
    scan = (rng.random((10, 10)) < 0.2).astype(np.int32)
    field = rng.integers(0, 9, (10, 10)).astype(np.int32)
    a = match_ref.expected_match(scan, field, window=2, field_max=9)
    b = match_ref.expected_match(scan, field, shift=(0, 0), pivot=(5, 5), rotations=[[UNIT, 0]], window=2, field_max=9)
    assert a["best"].tolist() == b["best"].tolist() and np.array_equal(a["scores"], b["scores"])
    # (16384, 16384): a rotation by 45 degrees that also stretches by sqrt(2): (dr, dc) -> (dr - dc, dr + dc), used as given
    rr, cc = match_ref.rotated_cells(scan, (5, 5), (UNIT, UNIT))
    r, c = np.nonzero(scan > 0)
    assert np.array_equal(rr, 5 + (r - 5) - (c - 5)) and np.array_equal(cc, 5 + (r - 5) + (c - 5))
    # the zero pair folds every cell onto the pivot, and every one counts
    zero = match_ref.expected_match(scan, field, rotations=[[0, 0]], window=0, field_max=9)
    assert zero["best"].tolist() == [0, 0, 0, int(field[5, 5]) * int(scan.sum()), int(scan.sum()), 1]


# ---------------------------------------------------------------- a drive: the wrong prior shift is recovered

def test_a_wrong_prior_shift_is_recovered_and_the_fusion_is_that_of_the_true_one():
    rng = np.random.default_rng(5)
    side, W = 30, 4
    world = rng.random((side + 20, side + 20)) < 0.06
    origins = [(10, 10), (12, 7), (9, 11)]  # the absolute cell of the window's cell (0, 0), frame by frame
    p = fusion_ref.params()
    off = np.array([2, -1])
    truth = corrected = None
    for f, (o0, o1) in enumerate(origins):
        state = np.where(world[o0: o0 + side, o1: o1 + side], 1, -1).astype(np.int32)
        if f == 0:
            truth = corrected = fusion_ref.expected_fusion(state, None, None, p)
            continue
        true_shift = np.array(origins[f]) - np.array(origins[f - 1])  # window cell (r, c) was cell (r, c) + true_shift of the frame before
        wrong = true_shift + off
        got = match_ref.expected_match(state, corrected["evidence"], shift=wrong, window=W, field_max=p["e_max"])["best"]
        assert got[:3].tolist() == [0, -2, 1] and got[5] == 1, f  # the correction undoes the offset, unambiguously
        fixed = wrong + got[1:3]
        assert fixed.tolist() == true_shift.tolist()
        corrected = fusion_ref.expected_fusion(state, corrected["evidence"], fixed, p)
        truth = fusion_ref.expected_fusion(state, truth["evidence"], true_shift, p)
        smeared = fusion_ref.expected_fusion(state, truth["evidence"], wrong, p)
        for key in ("evidence", "fused", "frontier", "counts"):
            assert np.array_equal(corrected[key], truth[key]), (f, key)
        assert not np.array_equal(smeared["evidence"], truth["evidence"])  # (what the correction is for)
