"""FRESH maps by the sign tag (groundgrid_amd/csrc/sweep_core.h sw_untag), checked without a GPU.

On a fresh launch k_patch stores its confidences with bit 31 set; the sweep makes the plain sweep's loads and takes a loaded cell as it is
iff the bit is set, else the slot's reset pair.  Everything else in the layer's memory is STALE: whatever the slot's last use left there --
positive confidences, always.  The host emulation (gg_debug_emulate_ring_sweep_fresh) builds that layer from a mask: 1 = written by k_patch in
this call (tagged), 0 = poison (a NaN with a clear sign bit), 2 = the caller's stale pair as it stands.  The existing tests
(test_sweep_emul_cpu.py) cover the poison; here the unmarked cells hold what a real slot holds: random positive finite pairs, large
magnitudes included, or the finished layer of an earlier call.  Whatever the stale memory and the interleaving of the wavefronts, the result
equals the oracle's serial sweep on the layer AS DEFINED (marked cells: their values; all others: the reset pair) bit for bit, no output
confidence has its sign bit set, and on maps with an odd number of rows the marked cells of ring c -- which no sweep visits -- keep their
values and lose the tag."""
import ctypes as C

import numpy as np
import pytest

from groundgrid_amd import _lib, build
from oracle import oracle

# n: 12 (the smallest), 66 / 69 (one ring group, even / odd), 130 / 131 (63 rings: a full group but for one lane), 134 / 135 (65 rings: two
# ring groups, the second with one lane -- the hand-over between groups), each as (length, resolution)
SIZES = [(12, 4.0, 0.33), (66, 33.0, 0.5), (69, 24.0, 0.35), (130, 43.0, 0.33), (131, 46.0, 0.35), (134, 67.0, 0.5), (135, 27.0, 0.2)]
SEEDS = (0, 1, 2, 3)
W_RESET = np.float32(0.0000001)


@pytest.fixture(scope="module")
def lib():
    build.build()
    L = C.CDLL(_lib.LIB_PATH)
    L.gg_debug_emulate_ring_sweep_fresh.restype = C.c_int
    L.gg_debug_emulate_ring_sweep_fresh.argtypes = [C.c_int, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_double, C.c_uint, C.POINTER(C.c_long)]
    return L


def emulate_fresh(L, n, resolution, ground, conf, mask, fresh_ground, base_z, decrease, seed):
    gp2 = np.empty((n * n, 2), dtype=np.float32)
    gp2[:, 0] = ground.ravel(order="F")
    gp2[:, 1] = conf.ravel(order="F")
    m = np.ascontiguousarray(mask.astype(np.uint8).ravel(order="F"))
    stats = (C.c_long * 8)()
    rc = L.gg_debug_emulate_ring_sweep_fresh(n, resolution, 12.0, gp2.ctypes.data, m.ctypes.data, fresh_ground, base_z, decrease, seed, stats)
    assert rc == 0, f"deadlock (-10), a plan fault (-11) or a stale cell with its sign bit set: {rc}"
    return gp2[:, 0].reshape((n, n), order="F"), gp2[:, 1].reshape((n, n), order="F")


def sign_bits(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 31) != 0


def patched_state(n, rng):
    """what k_patch may have written: rows and columns 2 .. n - 3, in clusters; its confidences are positive (0 allowed: the tag is a bit)"""
    ground = rng.normal(-1.7, 0.4, (n, n)).astype(np.float32)
    conf = rng.random((n, n)).astype(np.float32)
    conf[rng.random((n, n)) < 0.1] = 0.0
    conf[rng.random((n, n)) < 0.05] = 1.0
    patched = np.zeros((n, n), dtype=bool)
    for _ in range(max(3, n // 6)):
        i, j = rng.integers(2, n - 2, size=2)
        h, w = rng.integers(1, max(2, n // 4), size=2)
        patched[i:i + h, j:j + w] = True
    patched &= rng.random((n, n)) < 0.8
    patched[n - 3, 2:n - 2:3] = True  # (odd n: row n - 3 = c + c lies in ring c, which no sweep visits)
    patched[2:n - 2:4, n - 3] = True
    patched[:2, :] = patched[n - 2:, :] = False
    patched[:, :2] = patched[:, n - 2:] = False
    return ground, conf, patched


def reference(length, resolution, n, ground, conf, patched, fresh_ground, base_z):
    ref = oracle.OracleMap(length, resolution)
    assert ref.rows == n, (ref.rows, n)
    ref.set_layer("ground", np.where(patched, ground, fresh_ground).astype(np.float32))
    ref.set_layer("groundpatch", np.where(patched, conf, W_RESET).astype(np.float32))
    ref.stage_spiral(base_z)
    return ref, float(ref.cfg.occupied_cells_decrease_factor)


def check(n, g, w, ref, ground, conf, patched, what):
    assert not sign_bits(w).any(), (what, "a confidence came out with its sign bit set", np.argwhere(sign_bits(w))[:5].tolist())
    assert not np.isnan(g).any() and not np.isnan(w).any(), what
    assert np.array_equal(g, ref.layer("ground")), (what, np.argwhere(g != ref.layer("ground"))[:5].tolist())
    assert np.array_equal(w, ref.layer("groundpatch")), (what, np.argwhere(w != ref.layer("groundpatch"))[:5].tolist())
    if n % 2:  # the marked cells of ring c: their own values, untagged
        c = n // 2 - 1
        i, j = np.indices((n, n))
        border = patched & (np.maximum(np.abs(i - c), np.abs(j - c)) >= c)
        assert border.any(), "the case marks cells in ring c"
        assert np.array_equal(g[border], ground[border]) and np.array_equal(w[border].view(np.uint32), conf[border].view(np.uint32)), what


@pytest.mark.parametrize("n,length,resolution", SIZES)
def test_stale_memory_of_random_positive_pairs(lib, n, length, resolution):
    """unmarked cells hold random positive finite pairs, from denormals to the largest floats: never selected, whatever their magnitude"""
    rng = np.random.default_rng(4000 + n)
    fresh_ground, base_z = float(np.float32(rng.uniform(-0.5, 0.5))), -1.73
    ground, conf, patched = patched_state(n, rng)
    ref, decrease = reference(length, resolution, n, ground, conf, patched, np.float32(fresh_ground), base_z)
    exps = rng.uniform(-44.0, 38.5, (2, n, n))
    stale_g = np.minimum(10.0 ** exps[0], np.finfo(np.float32).max).astype(np.float32)
    stale_w = np.minimum(10.0 ** exps[1], np.finfo(np.float32).max).astype(np.float32)
    stale_w[rng.random((n, n)) < 0.2] = np.float32(0.5)  # (what the path leaves most often)
    assert np.isfinite(stale_g).all() and np.isfinite(stale_w).all() and not sign_bits(stale_w).any()
    mask = np.where(patched, 1, 2)
    for seed in SEEDS:
        g, w = emulate_fresh(lib, n, ref.resolution, np.where(patched, ground, stale_g), np.where(patched, conf, stale_w), mask, fresh_ground, base_z, decrease, seed)
        check(n, g, w, ref, ground, conf, patched, ("random stale pairs", n, seed))


@pytest.mark.parametrize("n,length,resolution", SIZES)
def test_stale_memory_of_an_earlier_call(lib, n, length, resolution):
    """unmarked cells hold the finished layer of an earlier call on another mask: after a complete call no cell carries the tag, so all of it
    reads as "not written in this call" """
    rng = np.random.default_rng(5000 + n)
    ground0, conf0, patched0 = patched_state(n, rng)
    z0 = float(np.float32(rng.uniform(-0.5, 0.5)))
    ref0, decrease = reference(length, resolution, n, ground0, conf0, patched0, np.float32(z0), -1.6)
    prev_g, prev_w = emulate_fresh(lib, n, ref0.resolution, ground0, conf0, patched0, z0, -1.6, decrease, 1)
    check(n, prev_g, prev_w, ref0, ground0, conf0, patched0, ("the earlier call", n))
    fresh_ground, base_z = float(np.float32(rng.uniform(-0.5, 0.5))), -1.73
    ground, conf, patched = patched_state(n, rng)
    ref, decrease = reference(length, resolution, n, ground, conf, patched, np.float32(fresh_ground), base_z)
    mask = np.where(patched, 1, 2)
    for seed in SEEDS:
        g, w = emulate_fresh(lib, n, ref.resolution, np.where(patched, ground, prev_g), np.where(patched, conf, prev_w), mask, fresh_ground, base_z, decrease, seed)
        check(n, g, w, ref, ground, conf, patched, ("an earlier call's layer", n, seed))


def test_a_stale_cell_with_its_sign_bit_set_is_refused(lib):
    """the emulation holds its caller to the rule the device path keeps: stale memory never carries the tag"""
    n, rng = 12, np.random.default_rng(6000)
    ground, conf, patched = patched_state(n, rng)
    stale_w = np.full((n, n), np.float32(0.5))
    stale_w[5, 5] = np.float32(-0.5)
    patched[5, 5] = False
    gp2 = np.empty((n * n, 2), dtype=np.float32)
    gp2[:, 0] = ground.ravel(order="F")
    gp2[:, 1] = np.where(patched, conf, stale_w).ravel(order="F")
    m = np.ascontiguousarray(np.where(patched, 1, 2).astype(np.uint8).ravel(order="F"))
    stats = (C.c_long * 8)()
    assert lib.gg_debug_emulate_ring_sweep_fresh(n, 0.33, 12.0, gp2.ctypes.data, m.ctypes.data, 0.0, -1.73, 10.0, 0, stats) != 0
