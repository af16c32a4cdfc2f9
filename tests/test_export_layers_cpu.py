"""gg_export_layers without a GPU: the entry point is declared, exported, bound and reachable from C and Python, and it refuses a null
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
    assert "gg_export_layers" in _lib.SYMBOLS
    assert hasattr(lib, "gg_export_layers")
    assert len(lib.gg_export_layers.argtypes) == 9
    assert lib.gg_abi_version() == 6


def test_a_c_program_calls_it_through_the_header():
    prog = r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_EXPORT_LAYERS) || GG_HAS_EXPORT_LAYERS != 1
    #error "GG_HAS_EXPORT_LAYERS"
    #endif
    int step(gg_context *ctx, float *d_dst, void *stream) {
        const int32_t slots[2] = {3, 1};
        const unsigned mask = (1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH);
        return gg_export_layers(ctx, 2, slots, 0, mask, GG_PLANES_COLMAJOR, d_dst, (size_t)364 * 364, stream)
             + gg_export_layers(ctx, 2, NULL, 4, mask, GG_PLANES_ROWMAJOR, d_dst, (size_t)364 * 364, NULL)
             + gg_export_layers(ctx, 2, NULL, 4, (1u << GG_NUM_LAYERS) - 1u, GG_PLANES_ROWMAJOR, d_dst, (size_t)364 * 364, GG_STREAM_DEFAULT);
    }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t.o")])


def test_null_context_is_invalid(lib):
    assert lib.gg_export_layers(None, 1, None, 0, 2, 0, None, 0, None) == -1  # GG_ERR_INVALID
    assert lib.gg_export_layers(None, 0, None, 0, 0, 0, None, 0, None) == -1


def test_python_entry_point_exists():
    assert callable(getattr(api.GroundSegmentation, "export_layers", None))
    params = inspect.signature(api.GroundSegmentation.export_layers).parameters
    for name in ("names", "slots", "first_slot", "n", "out", "row_major", "stream"):
        assert name in params, name
    assert params["names"].default is None and params["row_major"].default is False
    for name in ("slots", "first_slot", "n", "out", "row_major", "stream"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name


def test_score_configs_can_return_the_terrain():
    from groundgrid_amd import replay

    p = inspect.signature(replay.score_configs).parameters
    assert "return_ground" in p and p["return_ground"].default is False

