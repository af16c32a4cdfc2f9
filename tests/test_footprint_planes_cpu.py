"""gg_footprint_planes and gg_footprint_spans without a GPU: the entry points are declared, exported, bound and reachable from C and Python,
the ctypes mirror has the layout the C compiler gives the struct, the ABI version is what it was, a null context is refused before the
device is touched.  gg_footprint_spans (host arithmetic) is held word for word to tests/footprint_ref.py and to closed forms.  And the
expectation of the GPU tests (footprint_ref.expected_footprint: shifted copies of the padded blocked plane OR-ed together) is held without
the code under test: against scipy's binary dilation with the reflected structuring element, and on a single blocked cell."""
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
from tests import footprint_ref as ref  # noqa: E402

UNIT = ref.UNIT
INVALID = -1
FIELDS = ["n", "d_blocked", "blocked_stride", "spans", "n_headings", "radius", "min_fit", "outside_free", "order", "d_mask", "mask_stride", "d_fit",
          "fit_stride", "d_counts"]
SENTINEL = -77777


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


def c_spans(lib, rotations, rect, radius, give_spans=True, give_needed=True):
    """gg_footprint_spans as the C ABI has it: (status, table [K, 2 radius + 1, 2] prefilled with SENTINEL, needed or None)"""
    rot = np.ascontiguousarray(np.asarray(rotations, np.int32).reshape(-1, 2))
    K = rot.shape[0]
    table = np.full((K, 2 * max(radius, 0) + 1, 2), SENTINEL, np.int32)
    needed = C.c_int(SENTINEL)
    rc = lib.gg_footprint_spans(rot.ctypes.data_as(C.POINTER(C.c_int32)), K, (C.c_int32 * 4)(*[int(w) for w in rect]), radius,
                                table.ctypes.data_as(C.POINTER(C.c_int32)) if give_spans else None, C.byref(needed) if give_needed else None)
    return rc, table, needed.value if give_needed else None


# ---------------------------------------------------------------- the ABI

def test_symbols_are_exported_and_bound(lib):
    for name, n_args in (("gg_footprint_planes", 3), ("gg_footprint_spans", 6)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args


def test_struct_layout_equals_the_ctypes_mirror(lib):
    assert [f[0] for f in _lib.GGPlaneFootprints._fields_] == FIELDS
    lines = ['printf("%zu\\n", sizeof(gg_plane_footprints));'] + [f'printf("%zu\\n", offsetof(gg_plane_footprints, {k}));' for k in FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    assert [int(v) for v in out.split()] == [C.sizeof(_lib.GGPlaneFootprints)] + [getattr(_lib.GGPlaneFootprints, k).offset for k in FIELDS]


def test_feature_macro_and_the_limits_are_defined(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_FOOTPRINT_PLANES) || GG_HAS_FOOTPRINT_PLANES != 1
    #error "GG_HAS_FOOTPRINT_PLANES"
    #endif
    int main(void) { printf("%d %d %d %d\n", GG_HAS_FOOTPRINT_PLANES, GG_FOOTPRINT_MAX_HEADINGS, GG_FOOTPRINT_MAX_RADIUS, GG_ABI_VERSION); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, 32, 32, 6]
    assert (_lib.GG_HAS_FOOTPRINT_PLANES, _lib.GG_FOOTPRINT_MAX_HEADINGS, _lib.GG_FOOTPRINT_MAX_RADIUS) == (1, ref.MAX_HEADINGS, ref.MAX_RADIUS) == (1, 32, 32)
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION


def test_a_c_program_fills_the_struct_and_links(lib):
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int fits(gg_context *ctx, const int32_t *d_fused, const int32_t *table, uint32_t *d_mask, int32_t *d_fit, int32_t *d_counts, void *stream) {
        gg_plane_footprints x = {0};
        x.n = 2;
        x.d_blocked = d_fused;  x.blocked_stride = 364 * 364;
        x.spans = table;  x.n_headings = 32;  x.radius = 14;  x.min_fit = 1;  x.outside_free = 0;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_mask = d_mask;  x.mask_stride = 364 * 364;
        x.d_fit = d_fit;  x.fit_stride = 364 * 364;
        x.d_counts = d_counts;
        return gg_footprint_planes(ctx, &x, stream);
    }
    int main(void) {
        const int32_t identity[2] = {GG_MATCH_UNIT, 0}, rect[4] = {-GG_MATCH_UNIT, 2 * GG_MATCH_UNIT, 0, 0};
        int32_t spans[5][2];
        int needed = -9;
        if (gg_footprint_spans(identity, 1, rect, 2, &spans[0][0], &needed) != GG_OK) return 2;
        printf("%d", needed);
        for (int a = 0; a < 5; ++a) printf(" %d %d", spans[a][0], spans[a][1]);
        printf("\n");
        return fits(NULL, NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1;
    }
    ''')
    assert [int(v) for v in out.split()] == [2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]  # rows -1 .. 2 of column 0; row -2 is empty


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGPlaneFootprints()
    x.n = 1
    assert lib.gg_footprint_planes(None, C.byref(x), None) == INVALID
    assert lib.gg_footprint_planes(None, None, None) == INVALID
    x.n = 0
    assert lib.gg_footprint_planes(None, C.byref(x), None) == INVALID


def test_the_mirrored_constants_are_the_kernels():
    internal = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    assert int(re.search(r"constexpr int FOOTPRINT_MAX_HEADINGS = (\d+);", internal).group(1)) == _lib.GG_FOOTPRINT_MAX_HEADINGS
    assert int(re.search(r"constexpr int FOOTPRINT_MAX_RADIUS = (\d+);", internal).group(1)) == _lib.GG_FOOTPRINT_MAX_RADIUS
    assert int(re.search(r"constexpr int FOOTPRINT_TILE = (\d+);", internal).group(1)) == _lib.GG_FOOTPRINT_TILE
    assert _lib.GG_FOOTPRINT_RECT_LIMIT == ref.RECT_LIMIT == 2 ** 30
    # the seams of the GPU scenes lie on either side of every tile seam and of the 32-position halo word seams of a 128 x 128 plane
    T = _lib.GG_FOOTPRINT_TILE
    assert {T - 1, T}.issubset(ref.SEAMS) and {T // 2 - 1, T // 2, T + T // 2 - 1, T + T // 2}.issubset(ref.SEAMS)


def test_python_entry_points_exist():
    params = inspect.signature(api.GroundSegmentation.footprint_planes).parameters
    assert list(params)[:3] == ["self", "blocked", "spans"]
    defaults = {"min_fit": None, "outside_free": False, "order": "row", "mask": True, "fit": True, "counts": True, "out": None, "on_torch_stream": False}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is default or params[name].default == default, name
    params = inspect.signature(api.footprint_spans).parameters
    assert list(params) == ["rotations", "ahead", "behind", "left", "right", "pad", "radius"]
    assert params["pad"].default == ref.CAR_PAD == 0.7072 and params["radius"].default is None
    assert params["pad"].kind is inspect.Parameter.KEYWORD_ONLY and params["radius"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [f for f in api.FootprintOutputs.__dataclass_fields__] == ["mask", "fit", "counts"]


# ---------------------------------------------------------------- gg_footprint_spans against the restatement

THIN = (-3 * UNIT, 3 * UNIT, UNIT // 4, UNIT // 2)       # thinner than a cell and off the cell centres along the forward axis: empty rows
AWAY = (5 * UNIT, 9 * UNIT, -2 * UNIT, UNIT)             # does not hold the reference cell
SPAN_CASES = {
    "car K=1": (ref.headings(1), ref.rect_of(**ref.CAR)),
    "car K=3": (ref.headings(3), ref.rect_of(**ref.CAR)),
    "car K=32": (ref.headings(32), ref.rect_of(**ref.CAR)),
    "non-unit": ([(12000, -9000), (UNIT, 0), (-UNIT, UNIT)], ref.rect_of(**ref.CAR)),
    "zero pair, every cell": ([(0, 0)], (-5, 5, 0, 0)),
    "zero pair, no cell": ([(0, 0), (0, 0)], (1, 5, -3, 3)),
    "away": (ref.headings(8), AWAY),
    "thin": (ref.headings(16), THIN),
    "one cell": (ref.headings(5), (0, 0, 0, 0)),
    "needs 33": (ref.headings(4), (0, 33 * UNIT, 0, 0)),
    "needs 32": (ref.headings(4), (0, 32 * UNIT + UNIT // 2, 0, 0)),
    "the limit": ([(1, 0), (0, -1)], (-(1 << 30), 1 << 30, -(1 << 30), 1 << 30)),
}


@pytest.mark.parametrize("case", list(SPAN_CASES))
def test_spans_equal_the_restatement_word_for_word(lib, case):
    rotations, rect = SPAN_CASES[case]
    need = ref.needed_of(rotations, rect)
    # the pure query
    rc, table, needed = c_spans(lib, rotations, rect, 0, give_spans=False)
    assert (rc, needed) == (0, need) and np.all(table == SENTINEL), case
    for radius in sorted({min(max(need, 0), 32), min(max(need, 0) + 3, 32), 32}):
        rc, table, needed = c_spans(lib, rotations, rect, radius)
        want = ref.rect_spans(rotations, rect, radius)
        assert needed == need, case
        if want is None:  # cannot be represented in this radius: refused, the table untouched
            assert rc == INVALID and np.all(table == SENTINEL), (case, radius)
            continue
        assert rc == 0 and table.tolist() == want, (case, radius)
        assert ref.valid_table(table), (case, radius)  # row- and column-convex
        rc, again, needed = c_spans(lib, rotations, rect, radius, give_needed=False)  # `needed` is nullable
        assert rc == 0 and needed is None and np.array_equal(again, table)
    if need > 0:  # a radius smaller than needed
        rc, table, needed = c_spans(lib, rotations, rect, min(need - 1, 32))
        assert rc == INVALID and needed == need and np.all(table == SENTINEL), case


def test_what_the_span_cases_are_there_for():
    need = {case: ref.needed_of(*SPAN_CASES[case]) for case in SPAN_CASES}
    assert need["zero pair, every cell"] == 33 and need["zero pair, no cell"] == -1 and need["needs 33"] == 33 and need["needs 32"] == 32
    assert need["one cell"] == 0 and need["car K=32"] <= ref.CAR_RADIUS
    thin = np.array(ref.rect_spans(*SPAN_CASES["thin"], 32))
    empty = thin[..., 0] > thin[..., 1]
    assert empty.all(axis=1).any() and not empty.all()  # whole headings without a cell (the axis-aligned ones), and headings with cells
    assert all((0, 0) not in ref.rect_cells(pair, AWAY) for pair in SPAN_CASES["away"][0])
    assert all((0, 0) in ref.rect_cells(pair, SPAN_CASES["car K=32"][1]) for pair in SPAN_CASES["car K=32"][0])
    car = ref.car_spans()
    cells = set(ref.cells_of(car, 0))
    assert cells != {(-a, -b) for a, b in cells} and cells != {(b, a) for a, b in cells}  # asymmetric about its reference cell


def test_bad_arguments_of_spans_are_refused(lib):
    rect, rot = ref.rect_of(**ref.CAR), ref.headings(2)
    assert c_spans(lib, rot, rect, 14)[0] == 0
    for radius in (-1, 33):
        rc, table, _ = c_spans(lib, rot, rect, radius)
        assert rc == INVALID and np.all(table == SENTINEL)
    assert c_spans(lib, rot, rect, -1, give_spans=False)[0] == 0  # a pure query does not look at the radius
    for bad in ((UNIT + 1, 0), (0, -UNIT - 1), (-(1 << 31), 0)):
        assert c_spans(lib, [(UNIT, 0), bad], rect, 14)[0] == INVALID
    for bad in ((1, 0, 0, 0), (0, 0, 1, 0), ((1 << 30) + 1, (1 << 30) + 1, 0, 0), (0, 0, -(1 << 30) - 1, 0)):
        rc, table, needed = c_spans(lib, rot, bad, 14)
        assert rc == INVALID and np.all(table == SENTINEL) and needed == SENTINEL, bad
    table = np.zeros((1, 1, 2), np.int32)
    p, r4 = table.ctypes.data_as(C.POINTER(C.c_int32)), (C.c_int32 * 4)(0, 0, 0, 0)
    one = np.array([UNIT, 0], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.gg_footprint_spans(None, 1, r4, 0, p, None) == INVALID
    assert lib.gg_footprint_spans(one, 1, None, 0, p, None) == INVALID
    assert lib.gg_footprint_spans(one, 0, r4, 0, p, None) == INVALID
    assert lib.gg_footprint_spans(one, 33, r4, 0, p, None) == INVALID
    assert lib.gg_footprint_spans(one, 1, r4, 0, None, None) == 0  # nothing asked for, nothing wrong


def test_closed_forms(lib):
    """at the identity the set is the axis-aligned rectangle of cells; a quarter turn maps it by (a, b) -> (-b, a); a half turn reflects it"""
    rect = (-2 * UNIT - 100, 5 * UNIT + 100, -UNIT - 100, 3 * UNIT + 100)
    rc, table, needed = c_spans(lib, [(UNIT, 0), (0, UNIT), (-UNIT, 0)], rect, 6)
    assert rc == 0 and needed == 5
    identity = {(a, b) for a in range(-2, 6) for b in range(-1, 4)}
    assert set(ref.cells_of(table, 0)) == identity
    assert set(ref.cells_of(table, 1)) == {(-b, a) for a, b in identity}
    assert set(ref.cells_of(table, 2)) == {(-a, -b) for a, b in identity}


def test_python_spans(lib):
    rot = api.rotation_table([2.0 * np.pi * k / 32 for k in range(32)])
    assert rot.tolist() == [list(p) for p in ref.headings(32)]
    table = api.footprint_spans(rot, **ref.CAR, radius=ref.CAR_RADIUS)
    assert table.dtype == np.int32 and np.array_equal(table, ref.car_spans())
    tight = api.footprint_spans(rot, **ref.CAR)
    need = ref.needed_of(ref.headings(32), ref.rect_of(**ref.CAR))
    assert tight.shape == (32, 2 * need + 1, 2) and np.array_equal(tight, np.array(ref.rect_spans(ref.headings(32), ref.rect_of(**ref.CAR), need)))
    bare = api.footprint_spans(rot[:1], 2, 1, 0, 0, pad=0.0)  # the cells (-1 .. 2, 0)
    assert bare.tolist() == [[[1, 0], [0, 0], [0, 0], [0, 0], [0, 0]]]
    assert api.footprint_spans(rot[:1], 0.4, -0.2, 0, 0, pad=0.0).tolist() == [[[1, 0]]]  # no cell centre inside: radius 0, one empty row
    with pytest.raises(ValueError):
        api.footprint_spans(rot, **ref.CAR, radius=need - 1)
    with pytest.raises(ValueError):
        api.footprint_spans(rot, 40, 0, 0, 0)  # needs more than 32
    with pytest.raises(ValueError):
        api.footprint_spans(rot, **ref.CAR, radius=33)
    with pytest.raises(ValueError):
        api.footprint_spans(np.zeros((33, 2), np.int32), **ref.CAR)
    with pytest.raises(ValueError):
        api.footprint_spans(rot, float("nan"), 0, 0, 0)
    with pytest.raises(ValueError):
        api.footprint_spans(rot, 1, -3, 0, 0)  # behind the front: an empty rectangle


# ---------------------------------------------------------------- the expectation of the GPU tests, without the code under test

def small_spans():
    """a footprint for the 20 x 20 maps: 2 x 1 cells off the reference cell, 8 headings, R = 3"""
    return np.array(ref.rect_spans(ref.headings(8), ref.rect_of(2.0, 0.0, 0.5, 0.5, pad=0.3), 3), np.int32)


@pytest.mark.parametrize("side", [20, 67, 128])
@pytest.mark.parametrize("outside_free", [0, 1])
def test_restatement_equals_a_dilation(side, outside_free):
    """heading k does not fit at q iff q lies in the dilation of the blocked set by the reflected F_k (scipy's dilation reflects nothing:
    it ORs the input shifted by every offset of the structure about its centre, so the structure handed over is F_k mirrored)"""
    from scipy import ndimage

    spans = ref.car_spans() if side > 20 else small_spans()
    K, R = spans.shape[0], spans.shape[1] // 2
    for name in ("random", "seams", "rim"):
        blocked = ref.scene(name, side)
        got = ref.expected_footprint(blocked, spans, K, outside_free)
        pad = np.full((side + 2 * R, side + 2 * R), not outside_free, bool)
        pad[R: R + side, R: R + side] = blocked >= 0
        mask = np.zeros((side, side), np.uint32)
        for k in range(K):
            structure = np.zeros((2 * R + 1, 2 * R + 1), bool)
            for a, b in ref.cells_of(spans, k):
                structure[R - a, R - b] = True  # reflected
            if not structure.any():
                hit = np.zeros_like(pad)
            else:
                hit = ndimage.binary_dilation(pad, structure=structure, border_value=not outside_free)
            mask |= np.where(hit[R: R + side, R: R + side], 0, 1 << k).astype(np.uint32)
        assert np.array_equal(mask, got["mask"]), (name, side)
        p = np.array([bin(int(w)).count("1") for w in mask.ravel()]).reshape(side, side)
        assert np.array_equal(np.where(p >= K, -1, p), got["fit"]) and got["counts"].tolist() == [(p == K).sum(), (p >= K).sum(), (p == 0).sum()]


def test_a_single_blocked_cell():
    """with the outside free, bit k is clear exactly on {(r0 - a, c0 - b): (a, b) in F_k}: a reflected or transposed implementation differs,
    because the car is asymmetric about its reference cell"""
    side, spans = 67, ref.car_spans()
    blocked = ref.scene("one", side)
    (r0, c0), = [(int(r), int(c)) for r, c in zip(*np.nonzero(blocked >= 0))]
    assert (blocked >= 0).sum() == 1 and r0 != c0
    got = ref.expected_footprint(blocked, spans, 1, 1)
    for k in range(spans.shape[0]):
        clear = {(int(r), int(c)) for r, c in zip(*np.nonzero(((got["mask"] >> np.uint32(k)) & 1) == 0))}
        want = {(r0 - a, c0 - b) for a, b in ref.cells_of(spans, k)}
        assert all(0 <= r < side and 0 <= c < side for r, c in want)  # the cell is far enough from the border
        assert clear == want, k
        if k == 0:  # (a diagonal heading is its own transpose)
            assert clear != {(r0 + a, c0 + b) for a, b in ref.cells_of(spans, k)} and clear != {(r0 - b, c0 - a) for a, b in ref.cells_of(spans, k)}


@pytest.mark.parametrize("side", [67, 128])
@pytest.mark.parametrize("outside_free", [0, 1])
def test_the_random_scenes_hold_all_three_classes(side, outside_free):
    spans = ref.car_spans()
    K = spans.shape[0]
    p = ref.expected_footprint(ref.scene("random", side), spans, K, outside_free)["p"]
    classes = [int((p == K).sum()), int(((p > 0) & (p < K)).sum()), int((p == 0).sum())]
    print(f"side {side}, outside_free {outside_free}: p == K / 0 < p < K / p == 0 = {classes}")
    assert min(classes) >= 10, classes


def test_the_small_footprint_holds_all_three_classes_on_the_small_map():
    spans = small_spans()
    K = spans.shape[0]
    assert ref.valid_table(spans) and spans.shape == (8, 7, 2)
    blocked = ref.scene("random", 20)
    blocked[5, 7] = blocked[12, 3] = blocked[14, 15] = 0  # (1 % of 400 cells may be none)
    p = ref.expected_footprint(blocked, spans, K, 1)["p"]
    assert (p == K).sum() >= 10 and ((p > 0) & (p < K)).sum() >= 10 and (p == 0).sum() >= 3


def test_the_restatement_refuses_what_the_call_refuses():
    good = ref.car_spans()
    assert ref.valid_table(good)
    beyond = good.copy()
    beyond[0, 14] = (0, 15)
    hole = np.tile(np.array([[-1, 1], [1, 0], [-1, 1]], np.int32), (2, 1, 1))  # rows -1 and 1 without row 0: column 0 is not consecutive
    assert not ref.valid_table(beyond) and not ref.valid_table(hole)
    assert ref.valid_table(np.tile(np.array([[1, 0]], np.int32), (3, 1, 1)))  # all empty: fits everywhere
    e = ref.expected_footprint(ref.scene("full", 20), np.tile(np.array([[1, 0]], np.int32), (3, 1, 1)), 3, 0)
    assert e["counts"].tolist() == [400, 400, 0] and np.all(e["mask"] == 7) and np.all(e["fit"] == -1)
