"""gg_split_clouds without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirrors have the
layout the C compiler gives the two structs, the ABI version and gg_batch are what they were, and a null context is refused before the
device is touched."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from groundgrid_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_FIELDS = ["d_points", "d_height", "d_source"]
SPLIT_FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_labels", "d_label_masks",
                "ground", "nonground", "d_counts"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def compile_and_run(prog, lib_needed=True):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
        return subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, check=True).stdout.decode()


def test_symbol_is_exported_and_bound(lib):
    assert "gg_split_clouds" in _lib.SYMBOLS
    assert hasattr(lib, "gg_split_clouds")
    assert len(lib.gg_split_clouds.argtypes) == 3
    assert [f[0] for f in _lib.GGSplitSet._fields_] == SET_FIELDS
    assert [f[0] for f in _lib.GGCloudSplit._fields_] == SPLIT_FIELDS


def test_abi_version_and_gg_batch_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu\n", GG_ABI_VERSION, sizeof(gg_batch)); return 0; }
    ''')
    version, size = (int(v) for v in out.split())
    assert version == 6
    assert size == C.sizeof(_lib.GGBatch) == 120


def test_struct_layouts_equal_the_ctypes_mirrors(lib):
    lines = ['printf("%zu\\n", sizeof(gg_split_set));', 'printf("%zu\\n", sizeof(gg_cloud_split));']
    lines += [f'printf("%zu\\n", offsetof(gg_split_set, {k}));' for k in SET_FIELDS]
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_split, {k}));' for k in SPLIT_FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_SPLIT_CLOUDS) || GG_HAS_SPLIT_CLOUDS != 1
    #error "GG_HAS_SPLIT_CLOUDS"
    #endif
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    got = [int(v) for v in out.split()]
    want = [C.sizeof(_lib.GGSplitSet), C.sizeof(_lib.GGCloudSplit)]
    want += [getattr(_lib.GGSplitSet, k).offset for k in SET_FIELDS]
    want += [getattr(_lib.GGCloudSplit, k).offset for k in SPLIT_FIELDS]
    assert got == want


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int step(gg_context *ctx, const gg_point16 *d_points, const uint8_t *d_labels, gg_point16 *d_out, float *d_height, int32_t *d_counts, void *stream) {
        const int32_t slots[2] = {3, 1}, n_points[2] = {1000, 64};
        gg_cloud_split x = {0};
        x.n = 2;
        x.slots = slots;
        x.point_format = GG_POINT16;
        x.d_points = d_points;
        x.cloud_stride = 1024;
        x.n_points = n_points;
        x.d_labels = d_labels;
        x.nonground.d_points = d_out;
        x.nonground.d_height = d_height;
        x.d_counts = d_counts;
        int rc = gg_split_clouds(ctx, &x, stream);
        x.slots = NULL;
        x.first_slot = 4;
        x.d_labels = NULL;
        x.d_label_masks = d_labels;
        return rc + gg_split_clouds(ctx, &x, GG_STREAM_DEFAULT);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 2 * GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_is_invalid(lib):
    x = _lib.GGCloudSplit()
    x.n = 1
    assert lib.gg_split_clouds(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_split_clouds(None, None, None) == -1
    x.n = 0
    assert lib.gg_split_clouds(None, C.byref(x), None) == -1


def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.split_clouds).parameters
    assert list(params)[:3] == ["self", "points", "n_points"]
    defaults = {"labels": None, "masks": None, "transforms": None, "slots": None, "first_slot": 0, "ground": True, "nonground": True, "heights": True,
                "sources": True, "out": None}
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert params["on_torch_stream"].kind is inspect.Parameter.KEYWORD_ONLY
    fields = list(api.SplitOutputs.__dataclass_fields__)
    assert fields == ["counts"] + [f"{s}_{k}" for s in ("ground", "nonground") for k in ("points", "height", "source")]
    assert callable(api.SplitOutputs.clouds)
