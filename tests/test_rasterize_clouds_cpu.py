"""gg_rasterize_clouds without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version and gg_batch are what they were, and a null context is refused before the device is
touched."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from groundgrid_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RASTER_FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_labels", "d_label_masks",
                 "channel_mask", "order", "d_dst", "plane_stride"]
CHANNELS = ["NONGROUND_COUNT", "NONGROUND_MAX_HEIGHT", "NONGROUND_MIN_HEIGHT", "GROUND_COUNT", "GROUND_MAX_HEIGHT", "GROUND_MIN_HEIGHT"]


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


def test_symbol_is_exported_and_bound(lib):
    assert "gg_rasterize_clouds" in _lib.SYMBOLS
    assert hasattr(lib, "gg_rasterize_clouds")
    assert len(lib.gg_rasterize_clouds.argtypes) == 3
    assert [f[0] for f in _lib.GGCloudRaster._fields_] == RASTER_FIELDS


def test_channel_constants_equal_the_header(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_RASTERIZE_CLOUDS) || GG_HAS_RASTERIZE_CLOUDS != 1
    #error "GG_HAS_RASTERIZE_CLOUDS"
    #endif
    int main(void) { printf("%d ''' + " ".join(["%d"] * len(CHANNELS)) + r'''\n", GG_NUM_RASTER_CHANNELS, ''' + ", ".join("GG_RASTER_" + k for k in CHANNELS) + '''); return 0; }
    ''')
    got = [int(v) for v in out.split()]
    assert got == [6, 0, 1, 2, 3, 4, 5]
    assert _lib.GG_NUM_RASTER_CHANNELS == 6 == len(_lib.RASTER_CHANNELS)
    assert [getattr(_lib, "GG_RASTER_" + k) for k in CHANNELS] == got[1:]
    assert [k.upper() for k in _lib.RASTER_CHANNELS] == CHANNELS


def test_abi_version_and_gg_batch_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu %zu\n", GG_ABI_VERSION, sizeof(gg_batch), sizeof(gg_cloud_split)); return 0; }
    ''')
    version, size, split = (int(v) for v in out.split())
    assert version == 6
    assert size == C.sizeof(_lib.GGBatch) == 120
    assert split == C.sizeof(_lib.GGCloudSplit)


def test_struct_layout_equals_the_ctypes_mirror(lib):
    lines = ['printf("%zu\\n", sizeof(gg_cloud_raster));']
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_raster, {k}));' for k in RASTER_FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    got = [int(v) for v in out.split()]
    want = [C.sizeof(_lib.GGCloudRaster)] + [getattr(_lib.GGCloudRaster, k).offset for k in RASTER_FIELDS]
    assert got == want


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int step(gg_context *ctx, const gg_point16 *d_points, const uint8_t *d_labels, float *d_grid, void *stream) {
        const int32_t slots[2] = {3, 1}, n_points[2] = {1000, 64};
        gg_cloud_raster x = {0};
        x.n = 2;
        x.slots = slots;
        x.point_format = GG_POINT16;
        x.d_points = d_points;
        x.cloud_stride = 1024;
        x.n_points = n_points;
        x.d_labels = d_labels;
        x.channel_mask = 1u << GG_RASTER_NONGROUND_COUNT | 1u << GG_RASTER_NONGROUND_MAX_HEIGHT;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_dst = d_grid;
        x.plane_stride = 364 * 364;
        int rc = gg_rasterize_clouds(ctx, &x, stream);
        x.slots = NULL;
        x.first_slot = 4;
        x.d_labels = NULL;
        x.d_label_masks = d_labels;
        x.channel_mask = (1u << GG_NUM_RASTER_CHANNELS) - 1u;
        return rc + gg_rasterize_clouds(ctx, &x, GG_STREAM_DEFAULT);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL) == 2 * GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGCloudRaster()
    x.n = 1
    assert lib.gg_rasterize_clouds(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_rasterize_clouds(None, None, None) == -1
    x.n = 0
    assert lib.gg_rasterize_clouds(None, C.byref(x), None) == -1


def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.rasterize_clouds).parameters
    assert list(params)[:3] == ["self", "points", "n_points"]
    defaults = {"labels": None, "masks": None, "transforms": None, "slots": None, "first_slot": 0,
                "channels": ("nonground_count", "nonground_max_height"), "order": "row", "out": None, "on_torch_stream": True}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
