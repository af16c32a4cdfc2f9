"""gg_move_maps without a GPU: the entry point is declared, exported, bound and reachable from C and Python, and it refuses bad
arguments before it touches the device."""
import ctypes as C
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
    assert "gg_move_maps" in _lib.SYMBOLS
    assert hasattr(lib, "gg_move_maps")
    assert len(lib.gg_move_maps.argtypes) == 8


def test_a_c_program_calls_it_through_the_header():
    prog = r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_MOVE_MAPS) || GG_HAS_MOVE_MAPS != 1
    #error "GG_HAS_MOVE_MAPS"
    #endif
    int step(gg_context *ctx, void *stream) {
        const int32_t slots[2] = {3, 1};
        const double odom[4] = {1.0, 2.0, -0.5, 0.25};
        const double planes[8] = {0, 0, 1, 0, 0, 0, 1, 0};
        int32_t shifts[4];
        return gg_move_maps(ctx, 2, slots, 0, odom, planes, shifts, stream) + gg_move_maps(ctx, 2, NULL, 4, odom, planes, NULL, GG_STREAM_DEFAULT);
    }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t.o")])


def test_bad_arguments_without_a_context(lib):
    odom = (C.c_double * 2)(0.0, 0.0)
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, 0.0)
    assert lib.gg_move_maps(None, 1, None, 0, odom, plane, None, None) == -1  # GG_ERR_INVALID
    assert lib.gg_move_maps(None, 0, None, 0, None, None, None, None) == -1


def test_python_entry_point_exists():
    assert callable(getattr(api.GroundSegmentation, "move_maps", None))
    import inspect

    params = inspect.signature(api.GroundSegmentation.move_maps).parameters
    for name in ("odoms", "base_to_maps", "slots", "first_slot", "rotation", "on_torch_stream", "stream"):
        assert name in params, name
