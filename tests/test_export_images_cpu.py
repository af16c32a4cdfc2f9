"""gg_export_images without a GPU: the entry point is declared, exported, bound and reachable from C and Python, and it refuses a null
context before it touches the device."""
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


def test_symbol_is_exported_and_bound(lib):
    assert "gg_export_images" in _lib.SYMBOLS
    assert hasattr(lib, "gg_export_images")
    assert len(lib.gg_export_images.argtypes) == 3
    assert lib.gg_abi_version() == 6
    assert (_lib.GG_TERRAIN_HWC, _lib.GG_TERRAIN_CHW) == (0, 1)
    names = [f[0] for f in _lib.GGImageExport._fields_]
    assert names == ["n", "first_slot", "slots", "layer_mask", "d_images", "image_stride", "d_bounds", "d_terrain", "terrain_stride", "terrain_layout"]


def test_a_c_program_fills_the_struct_and_links(lib):
    prog = r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_EXPORT_IMAGES) || GG_HAS_EXPORT_IMAGES != 1
    #error "GG_HAS_EXPORT_IMAGES"
    #endif
    int step(gg_context *ctx, uint8_t *d_images, float *d_bounds, float *d_terrain, void *stream) {
        const int32_t slots[2] = {3, 1};
        gg_image_export x = {0};
        x.n = 2;
        x.slots = slots;
        x.layer_mask = (1u << GG_LAYER_GROUND) | (1u << GG_LAYER_POINTSRAW);
        x.d_images = d_images;
        x.image_stride = (size_t)364 * 364 + 37;
        x.d_bounds = d_bounds;
        x.d_terrain = d_terrain;
        x.terrain_stride = (size_t)3 * 364 * 364;
        x.terrain_layout = GG_TERRAIN_CHW;
        int rc = gg_export_images(ctx, &x, stream);
        x.slots = NULL;
        x.first_slot = 4;
        x.layer_mask = 0;
        x.terrain_layout = GG_TERRAIN_HWC;
        return rc + gg_export_images(ctx, &x, GG_STREAM_DEFAULT);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL) == 2 * GG_ERR_INVALID ? 0 : 1; }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])


def test_null_context_is_invalid(lib):
    x = _lib.GGImageExport()
    x.n = 1
    x.layer_mask = 2
    assert lib.gg_export_images(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_export_images(None, None, None) == -1
    x.n = 0
    assert lib.gg_export_images(None, C.byref(x), None) == -1


def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.export_images).parameters
    assert list(params)[:2] == ["self", "names"]
    assert params["names"].default is None
    defaults = {"terrain": False, "chw": False, "slots": None, "first_slot": 0, "n": None, "out": None, "on_torch_stream": False}
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.ImageExport.__dataclass_fields__] == ["images", "bounds", "terrain"]
