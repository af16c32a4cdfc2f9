"""gg_export_slopes without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the constants are the
header's, the ABI version and gg_batch are what they were, a null context is refused before the device is touched, and the numpy form of
the definition (tests/slopes_ref.py, what the GPU tests hold the kernels to) gives the hand-checkable answers."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

from groundgrid_amd import _lib, api, build
from tests.slopes_ref import CHANNELS as REF_CHANNELS, FRESH, slopes_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = ["GRAD_X", "GRAD_Y", "TANGENT", "NORMAL_Z", "STEP", "MIN_CONFIDENCE"]


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbol_is_exported_and_bound(lib):
    assert "gg_export_slopes" in _lib.SYMBOLS
    assert hasattr(lib, "gg_export_slopes")
    assert len(lib.gg_export_slopes.argtypes) == 9
    assert [str(t) for t in lib.gg_export_slopes.argtypes] == [str(t) for t in lib.gg_export_layers.argtypes]


def test_channel_constants_equal_the_header(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_EXPORT_SLOPES) || GG_HAS_EXPORT_SLOPES != 1
    #error "GG_HAS_EXPORT_SLOPES"
    #endif
    int main(void) { printf("%d ''' + " ".join(["%d"] * len(CHANNELS)) + r'''\n", GG_NUM_SLOPE_CHANNELS, ''' + ", ".join("GG_SLOPE_" + k for k in CHANNELS) + '''); return 0; }
    ''')
    got = [int(v) for v in out.split()]
    assert got == [6, 0, 1, 2, 3, 4, 5]
    assert _lib.GG_NUM_SLOPE_CHANNELS == 6 == len(_lib.SLOPE_CHANNELS)
    assert [getattr(_lib, "GG_SLOPE_" + k) for k in CHANNELS] == got[1:]
    assert _lib.SLOPE_CHANNELS == ["grad_x", "grad_y", "tangent", "normal_z", "step", "min_confidence"] == REF_CHANNELS
    assert [k.upper() for k in _lib.SLOPE_CHANNELS] == CHANNELS


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


def test_a_c_program_calls_it_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int planes(gg_context *ctx, float *d_dst, void *stream) {
        const int32_t slots[2] = {3, 1};
        int rc = gg_export_slopes(ctx, 2, slots, 0, 1u << GG_SLOPE_TANGENT | 1u << GG_SLOPE_STEP, GG_PLANES_ROWMAJOR, d_dst, 364 * 364 + 1, stream);
        return rc + gg_export_slopes(ctx, 4, NULL, 2, (1u << GG_NUM_SLOPE_CHANNELS) - 1u, GG_PLANES_COLMAJOR, d_dst, 364 * 364, GG_STREAM_DEFAULT);
    }
    int main(void) { return planes(NULL, NULL, NULL) == 2 * GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_is_invalid(lib):
    assert lib.gg_export_slopes(None, 1, None, 0, 0x3F, 0, None, 0, None) == -1  # GG_ERR_INVALID
    assert lib.gg_export_slopes(None, 0, None, 0, 0, 0, None, 0, None) == -1
    assert lib.gg_export_slopes(None, -1, None, 0, 0x3F, 1, None, 1 << 20, None) == -1


def test_python_entry_point_has_the_signature_of_export_layers():
    params = inspect.signature(api.GroundSegmentation.export_slopes).parameters
    assert list(params)[:2] == ["self", "names"]
    assert params["names"].default is None and params["names"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    defaults = {"slots": None, "first_slot": 0, "n": None, "out": None, "row_major": False, "stream": None, "own_stream": False, "plane_stride": None}
    assert list(params)[2:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    layers = inspect.signature(api.GroundSegmentation.export_layers).parameters
    assert list(layers) == list(params)


# ---------------------------------------------------------------- the definition in numpy

def test_reference_on_a_ramp_follows_the_row_and_column_convention():
    # z = a x + b y with x = -res * row, y = -res * col (rows grow towards -x, columns towards -y)
    rows, cols, res, a, b = 9, 7, np.float32(0.5), 0.25, -0.125
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    g = (a * (-0.5 * r) + b * (-0.5 * c)).astype(np.float32)  # (every value is a multiple of 1 / 16: exact)
    w = np.full((rows, cols), 0.75, np.float32)
    gx, gy, tangent, normal_z, step, conf = slopes_reference(g, w, res)
    assert np.all(gx == np.float32(a)) and np.all(gy == np.float32(b))  # one-sided on the border, the same there
    assert np.all(tangent == np.sqrt(np.float32(a * a + b * b)))
    assert np.allclose(normal_z, 1.0 / np.sqrt(1.0 + a * a + b * b), rtol=1e-6, atol=0)
    # the largest step is to the diagonal neighbour: (|a| + |b|) * res
    assert np.all(step[1:-1, 1:-1] == np.float32((abs(a) + abs(b)) * 0.5))
    assert np.all(conf == np.float32(0.75))
    # a general ramp: within float rounding of the differences
    g = (0.3 * (-0.33 * r) - 0.7 * (-0.33 * c) + 1.5).astype(np.float32)
    gx, gy = slopes_reference(g, w, np.float32(0.33))[:2]
    assert np.allclose(gx, 0.3, rtol=0, atol=2e-6) and np.allclose(gy, -0.7, rtol=0, atol=2e-6)
    # the sign: the ground rises towards +x = towards smaller rows
    g = np.zeros((5, 5), np.float32)
    g[0, :] = 1.0
    gx = slopes_reference(g, np.ones_like(g), np.float32(1.0))[0]
    assert np.all(gx[0] == 1.0) and np.all(gx[1] == 0.5) and np.all(gx[2:] == 0.0)


def test_reference_on_a_single_raised_cell():
    g = np.zeros((7, 8), np.float32)
    g[3, 4] = 2.0
    w = np.full(g.shape, 0.5, np.float32)
    w[0, 0] = 0.125
    w[6, 7] = np.nan
    gx, gy, tangent, normal_z, step, conf = slopes_reference(g, w, np.float32(0.5))
    want = np.zeros_like(g)
    want[2:5, 3:6] = 2.0  # the ring and the cell itself
    assert np.array_equal(bits(step), bits(want))
    want_gx = np.zeros_like(g)
    want_gx[4, 4], want_gx[2, 4] = 2.0, -2.0  # (g(r-1) - g(r+1)) / (2 * 0.5)
    assert np.array_equal(gx, want_gx)
    assert gy[3, 5] == 2.0 and gy[3, 3] == -2.0 and gy[3, 4] == 0.0
    assert tangent[4, 4] == 2.0 and normal_z[4, 4] == np.float32(1.0) / np.sqrt(np.float32(5.0))
    want_conf = np.full(g.shape, 0.5, np.float32)
    want_conf[0:2, 0:2] = 0.125
    assert np.array_equal(bits(conf), bits(want_conf))  # (the NaN is skipped, its own cell included: the others are numbers)


def test_reference_nan_and_inf_rules():
    g = np.zeros((5, 5), np.float32)
    g[2, 2] = np.nan
    g[0, 4] = g[2, 4] = np.inf
    w = np.full(g.shape, np.nan, np.float32)
    w[4, 4] = 0.25
    gx, gy, tangent, normal_z, step, conf = slopes_reference(g, w, np.float32(1.0))
    assert np.isnan(gx[1, 2]) and np.isnan(gx[3, 2]) and not np.isnan(gx[2, 2])  # (the centre is not in its own gradient stencil)
    assert np.isnan(gy[2, 1]) and np.isnan(gy[2, 3])
    assert not np.isnan(step).any() and not np.signbit(step).any()
    assert step[2, 2] == 0.0 and step[1, 1] == 0.0  # every difference at the NaN cell is NaN: skipped
    assert step[0, 3] == np.inf and step[0, 4] == np.inf and step[1, 4] == np.inf
    assert np.isnan(gx[1, 4]) and gx[0, 4] == np.inf  # inf - inf; one-sided on the border row: inf - 0
    assert np.isnan(conf[:3, :3]).all() and np.all(conf[3:, 3:] == 0.25)


def test_reference_on_a_constant_plane_gives_the_fresh_map_constants():
    for z in (0.0, -1.5, 0.3):
        g = np.full((6, 5), z, np.float32)
        w = np.full((6, 5), 1e-7, np.float32)
        planes = slopes_reference(g, w, np.float32(0.33))
        for k, (p, want) in enumerate(zip(planes, FRESH)):
            assert np.all(bits(p) == bits(want)), (z, k)
    assert [int(bits(v)[0]) for v in FRESH] == [0, 0, 0, 0x3F800000, 0, int(bits(np.float32(1e-7))[0])]
