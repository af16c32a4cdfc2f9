"""gg_import_layers without a GPU: the entry point is declared, exported, bound and reachable from C and Python, and it refuses a null
context before it touches the device."""
import inspect
import os
import subprocess
import tempfile

import pytest

from groundgrid_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbol_is_exported_and_bound(lib):
    assert "gg_import_layers" in _lib.SYMBOLS
    assert hasattr(lib, "gg_import_layers")
    assert len(lib.gg_import_layers.argtypes) == 9
    assert lib.gg_abi_version() == 6


def test_a_c_program_calls_it_through_the_header():
    prog = r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_IMPORT_LAYERS) || GG_HAS_IMPORT_LAYERS != 1
    #error "GG_HAS_IMPORT_LAYERS"
    #endif
    int step(gg_context *ctx, const float *d_src, void *stream) {
        const int32_t slots[2] = {3, 1};
        const unsigned mask = (1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH);
        return gg_import_layers(ctx, 2, slots, 0, mask, GG_PLANES_COLMAJOR, d_src, (size_t)364 * 364, stream)
             + gg_import_layers(ctx, 2, NULL, 4, mask, GG_PLANES_ROWMAJOR, d_src, (size_t)364 * 364 + 37, NULL)
             + gg_import_layers(ctx, 2, NULL, 4, (1u << GG_NUM_LAYERS) - 1u, GG_PLANES_ROWMAJOR, d_src, (size_t)364 * 364, GG_STREAM_DEFAULT);
    }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t.o")])


def test_null_context_is_invalid(lib):
    assert lib.gg_import_layers(None, 1, None, 0, 2, 0, None, 0, None) == -1  # GG_ERR_INVALID
    assert lib.gg_import_layers(None, 0, None, 0, 0, 0, None, 0, None) == -1


def test_python_entry_points_exist():
    cls = api.GroundSegmentation
    params = inspect.signature(cls.import_layers).parameters
    assert list(params)[:3] == ["self", "planes", "names"]
    assert params["names"].default is None
    defaults = {"slots": None, "first_slot": 0, "n": None, "row_major": False, "stream": None, "own_stream": False, "plane_stride": None}
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    snap = inspect.signature(cls.snapshot_maps).parameters
    assert list(snap) == ["self", "slots", "first_slot", "n"]
    assert snap["slots"].default is None and snap["first_slot"].default == 0 and snap["n"].default is None
    rest = inspect.signature(cls.restore_maps).parameters
    assert list(rest) == ["self", "state", "slots", "first_slot"]
    assert rest["slots"].default is None and rest["first_slot"].default == 0
