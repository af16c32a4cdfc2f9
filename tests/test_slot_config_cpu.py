"""gg_set_slot_configs / gg_get_slot_config without a GPU: both entry points are declared, exported, bound and reachable from C and
Python, and they refuse bad arguments before they touch the device."""
import ctypes as C
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


def test_symbols_are_exported_and_bound(lib):
    P = C.POINTER
    for name in ("gg_set_slot_configs", "gg_get_slot_config"):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert lib.gg_set_slot_configs.argtypes == [C.c_void_p, C.c_int, P(C.c_int32), C.c_int, P(_lib.GGConfig)]
    assert lib.gg_get_slot_config.argtypes == [C.c_void_p, C.c_int, P(_lib.GGConfig), P(C.c_int)]


def test_a_c_program_calls_them_through_the_header():
    prog = r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_SLOT_CONFIG) || GG_HAS_SLOT_CONFIG != 1
    #error "GG_HAS_SLOT_CONFIG"
    #endif
    int configure(gg_context *ctx) {
        gg_config cfgs[2];
        gg_default_config(&cfgs[0]);
        gg_default_config(&cfgs[1]);
        cfgs[1].max_ring = 31;
        const int32_t slots[2] = {3, 1};
        int own = 0;
        gg_config got;
        return gg_set_slot_configs(ctx, 2, slots, 0, cfgs) + gg_set_slot_configs(ctx, 2, NULL, 4, NULL) +
               gg_get_slot_config(ctx, 3, &got, &own) + gg_get_slot_config(ctx, 1, &got, NULL) + own;
    }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t.o")])


def test_bad_arguments_without_a_context(lib):
    cfg = _lib.GGConfig()
    lib.gg_default_config(C.byref(cfg))
    own = C.c_int(7)
    assert lib.gg_set_slot_configs(None, 1, None, 0, C.byref(cfg)) == -1  # GG_ERR_INVALID
    assert lib.gg_set_slot_configs(None, 0, None, 0, None) == -1
    assert lib.gg_set_slot_configs(None, -1, None, 0, None) == -1
    assert lib.gg_get_slot_config(None, 0, C.byref(cfg), C.byref(own)) == -1
    assert own.value == 7


def test_python_entry_points_exist():
    params = inspect.signature(api.GroundSegmentation.set_slot_configs).parameters
    for name in ("configs", "slots", "first_slot"):
        assert name in params, name
    assert callable(getattr(api.GroundSegmentation, "slot_config", None))
    assert callable(getattr(api.GridMap, "setConfig", None)) and callable(getattr(api.GridMap, "getConfig", None))
