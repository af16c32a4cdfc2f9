"""gg_export_layers (the layers of many maps as dense planes in device memory, one launch) on the device: bit for bit what gg_get_layers
returns per map and what the CPU oracle holds -- fresh maps, lazily kept layers, caller streams, GG_FLAG_CONCURRENT_HALVES, per-map
configurations -- and errors that change nothing.  Every comparison is on bits; there is no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402
from groundgrid_amd._lib import LAYERS  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

LAZY = ["maxGroundHeight", "groundCandidates", "planeDist"]
PERCALL = [k for k in LAYERS if k not in ("ground", "groundpatch")]
MASKS = [["ground"], ["ground", "groundpatch"], list(LAYERS), ["points", "minGroundHeight", "m2", "pointsRaw", "variance"], LAZY]
SENTINEL = 0x7FC12345  # (a NaN payload no layer holds)
POSE = (0.3, 0.2, 1.5, 0.02, -0.01, 0.3, 0.95)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def batch_points(clouds, stride):
    import torch

    host = np.zeros((len(clouds), stride), dtype=api.POINT16_DTYPE)
    for b, c in enumerate(clouds):
        host[b, : len(c)] = api.pack16(c)
    return torch.from_numpy(host.view(np.uint8).reshape(len(clouds), stride, 16)).cuda()


def stride_of(clouds):
    return (max(len(c) for c in clouds) + 63) // 64 * 64


def mask_of(names):
    return sum(1 << LAYERS.index(k) for k in names)


def fresh_count(seg):
    return seg.debug_set_tuning("fresh_count", 0)


def sentinel_tensor(count):
    import torch

    return torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def raw_export(seg, n, slots, first_slot, mask, order, dst_ptr, plane_stride, stream=None):
    """gg_export_layers as the C ABI has it; returns the status"""
    import torch

    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_export_layers(seg._ctx, n, sl, first_slot, mask, order, C.c_void_p(dst_ptr) if dst_ptr else None, plane_stride,
                                   C.c_void_p(s if s else _lib.GG_STREAM_DEFAULT))


def plane_of(flat, seg, i, K, k, stride, row_major):
    """plane k of map i of a downloaded destination as a (rows, cols) array"""
    p = flat[(i * K + k) * stride: (i * K + k) * stride + seg.rows * seg.cols]
    return p.reshape(seg.rows, seg.cols) if row_major else p.reshape((seg.rows, seg.cols), order="F")


def assert_export_equals(planes, seg, slots, names, want_of, tag, row_major=False):
    """planes: the tensor export_layers returned, on the host; want_of(slot) -> {layer: (rows, cols) array}"""
    for i, s in enumerate(slots):
        want = want_of(s)
        for k, name in enumerate(names):
            got = planes[i, k] if row_major else planes[i, k].T
            assert same_bits(got, want[name]), f"{tag}: map {i} (slot {s}) layer {name}: {int((bits(got) != bits(want[name])).sum())} cells differ"


def warm_maps(seg, slots, seed, frames=2, n_az=150, refs=None, eager=False):
    """`frames` batches of distinct clouds on `slots`, a scroll in front of every batch but the first: warm, scrolled, non-fresh maps"""
    import torch

    K = len(slots)
    base = [synth.hdl64_cloud(seed=seed + k, n_az=n_az + 9 * k) for k in range(K)]
    stride = stride_of(base)
    for f in range(frames):
        odoms = np.array([(0.9 * f * (1 + k % 3), -0.7 * f * (k % 2)) for k in range(K)])
        clouds = []
        for k in range(K):
            c = synth.clone_cloud(base[(k + f) % K])
            c["x"] += np.float32(odoms[k][0])
            c["y"] += np.float32(odoms[k][1])
            clouds.append(c)
        origins = np.array([(odoms[k][0], odoms[k][1], 0.0) for k in range(K)], dtype=np.float32)
        if f:
            seg.move_maps(odoms, [POSE] * K, slots=slots, on_torch_stream=True)
        seg.filter_batch(batch_points(clouds, stride), [len(c) for c in clouds], origins, np.full(K, -1.73), slots=slots)
        torch.cuda.synchronize()
        if refs is not None:
            for k in range(K):
                if f:
                    refs[k].update(odoms[k][0], odoms[k][1], POSE)
                refs[k].filter_cloud(clouds[k], tuple(origins[k]), -1.73)


# ---------------------------------------------------------------- 1. parity with gg_get_layers

@pytest.mark.parametrize("variant", [0, 1])  # (0: the tiled kernel, 1: the destination-ordered gather)
@pytest.mark.parametrize("length,res,n_slots,size", [(120.0, 0.33, 10, 364), (200.0, 0.2, 3, 1000), (26.0, 0.33, 5, 79)])
def test_parity_with_the_getter(length, res, n_slots, size, variant):
    import torch

    seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=20000)
    assert seg.rows == seg.cols == size
    seg.debug_set_tuning("export_variant", variant)
    seg.reset_maps(odom_z=0.3)
    written = list(range(1, n_slots))  # (slot 0 stays as the reset left it)
    warm_maps(seg, written, seed=1200)
    C_ = seg.rows * seg.cols
    stride = C_ + 37
    rng = np.random.default_rng(9)
    subset = [int(s) for s in rng.permutation(n_slots)[: max(2, n_slots - 1)]]
    if 0 not in subset:
        subset[-1] = 0  # (the fresh map is in the permuted list)
    selections = [(subset, 0, len(subset)), (None, 1, n_slots - 1)]
    fresh_before = fresh_count(seg)
    got = []
    for names in MASKS:
        for row_major in (False, True):
            for slots, first, n in selections:
                K = len(names)
                dst = sentinel_tensor(n * K * stride)
                order = _lib.GG_PLANES_ROWMAJOR if row_major else _lib.GG_PLANES_COLMAJOR
                assert raw_export(seg, n, slots, first, mask_of(names), order, dst.data_ptr(), stride) == 0, seg._L.gg_last_error(seg._ctx)
                got.append((names, row_major, slots if slots is not None else list(range(first, first + n)), dst))
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    host = [(names, rm, sl, dst.cpu().numpy()) for names, rm, sl, dst in got]
    want = {s: seg.map(s).layers() for s in range(n_slots)}  # (the getter runs AFTER every export: its fills cannot have helped them)
    for names, row_major, sl, flat in host:
        K = len(names)
        tag = f"{size} {'+'.join(names) if K < 11 else 'all'} {'row' if row_major else 'col'}-major"
        for i, s in enumerate(sl):
            for k, name in enumerate(names):
                p = plane_of(flat, seg, i, K, k, stride, row_major)
                assert same_bits(p, want[s][name]), f"{tag}: map {i} (slot {s}) layer {name}: {int((bits(p) != bits(want[s][name])).sum())} cells differ"
                gap = flat[(i * K + k) * stride + C_: (i * K + k + 1) * stride]
                assert np.all(gap.view(np.uint32) == SENTINEL), f"{tag}: the gap behind plane {k} of map {i} was written"
    seg.close()


def test_python_entry_point_shapes_and_out():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.reset_maps(odom_z=0.1)
    warm_maps(seg, [2, 0, 3], seed=1300, frames=1)
    a = seg.export_layers()
    assert a.shape == (4, 11, seg.cols, seg.rows) and a.dtype == torch.float32 and a.is_cuda
    b = seg.export_layers(["ground", "pointsRaw"], slots=[3, 0], row_major=True)
    assert b.shape == (2, 2, seg.rows, seg.cols)
    out = torch.zeros((2, 1, seg.cols, seg.rows), dtype=torch.float32, device="cuda")
    assert seg.export_layers(["groundpatch"], first_slot=2, n=2, out=out) is out
    with pytest.raises(ValueError):
        seg.export_layers(["groundpatch", "ground"])
    torch.cuda.synchronize()
    a, b, out = a.cpu().numpy(), b.cpu().numpy(), out.cpu().numpy()
    want = {s: seg.map(s).layers() for s in range(4)}
    assert_export_equals(a, seg, [0, 1, 2, 3], list(LAYERS), lambda s: want[s], "all")
    assert_export_equals(b, seg, [3, 0], ["ground", "pointsRaw"], lambda s: want[s], "row-major", row_major=True)
    assert_export_equals(out, seg, [2, 3], ["groundpatch"], lambda s: want[s], "out")
    seg.close()


# ---------------------------------------------------------------- 2. against the oracle directly

@pytest.mark.parametrize("variant", [0, 1])
def test_against_the_oracle(variant):
    import torch

    slots = [3, 0, 5, 2]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    seg.debug_set_tuning("export_variant", variant)  # (0: the tiled kernel, 1: the destination-ordered gather -- the same planes)
    for s in slots:
        seg.map(s).reset()
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    warm_maps(seg, slots, seed=1400, frames=3, refs=refs)
    for row_major in (False, True):
        planes = seg.export_layers(slots=slots, row_major=row_major)
        torch.cuda.synchronize()
        planes = planes.cpu().numpy()
        for i, s in enumerate(slots):
            for k, name in enumerate(LAYERS):
                got = planes[i, k] if row_major else planes[i, k].T
                want = refs[i].layer(name)
                assert np.array_equal(got, want, equal_nan=True), f"slot {s} layer {name} row_major={row_major}: {int((got != want).sum())} cells differ"
    seg.close()


# ---------------------------------------------------------------- 3. fresh maps

def test_fresh_maps_stay_fresh():
    import torch

    B = 100
    clouds = [synth.hdl64_cloud(seed=1500 + k, n_az=96 + (k % 5) * 3) for k in range(B)]
    stride = stride_of(clouds)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    z = [0.25 if s < 50 else -1.5 for s in range(B)]
    seg.reset_maps(0, 50, odom_z=0.25, on_torch_stream=True)
    seg.reset_maps(50, 50, odom_z=-1.5, on_torch_stream=True)
    refs = [oracle.OracleMap(120.0, 0.33, odom_z=z[s]) for s in range(B)]
    assert fresh_count(seg) == B
    for row_major, variant in ((False, 0), (True, 0), (False, 1), (True, 1)):
        seg.debug_set_tuning("export_variant", variant)
        planes = seg.export_layers(["ground", "groundpatch"], row_major=row_major)
        torch.cuda.synchronize()
        assert fresh_count(seg) == B
        planes = planes.cpu().numpy()
        for s in range(B):
            assert np.all(bits(planes[s, 0]) == bits(np.float32(z[s]))), s
            assert np.all(bits(planes[s, 1]) == bits(np.float32(1e-7))), s
    # three maps are written (a launch too small for the fresh path fills them first); the other 97 stay fresh
    first = [7, 60, 99]
    pts_all = batch_points(clouds, stride)
    origins = np.array([[0.05 * (b % 7), -0.03 * (b % 5), 0.01 * (b % 3)] for b in range(B)], dtype=np.float32)
    base_z = np.array([-1.73 + 0.003 * (b % 9) for b in range(B)])
    seg.filter_batch(pts_all[first].contiguous(), [len(clouds[s]) for s in first], origins[first], base_z[first], slots=first)
    for s in first:
        refs[s].filter_cloud(clouds[s], tuple(origins[s]), float(base_z[s]))
    assert fresh_count(seg) == B - 3
    mixed = [7, 8, 60, 61, 99, 0]
    mixed_names = ["ground", "groundpatch", "minGroundHeight", "pointsRaw"]
    for variant in (1, 0):
        seg.debug_set_tuning("export_variant", variant)
        planes = seg.export_layers(mixed_names, slots=mixed)
        torch.cuda.synchronize()
        assert fresh_count(seg) == B - 3
        assert_export_equals(planes.cpu().numpy(), seg, mixed, mixed_names, lambda s: {k: refs[s].layer(k) for k in mixed_names},
                             f"mixed fresh and written, variant {variant}")
    # The 97 maps the exports left fresh (asserted above: the flags are what an export could have disturbed) go through a batch large
    # enough for the launcher's fresh path, and match the oracle.  That the launcher took that path is its own decision from those flags;
    # fresh_count falls to 0 either way.
    rest = [s for s in range(B) if s not in first]
    out = seg.filter_batch(pts_all[rest].contiguous(), [len(clouds[s]) for s in rest], origins[rest], base_z[rest], slots=rest)
    assert fresh_count(seg) == 0
    planes = seg.export_layers(["ground", "groundpatch"], slots=rest)
    torch.cuda.synchronize()
    labels, planes = out.labels.cpu().numpy(), planes.cpu().numpy()
    for b, s in enumerate(rest):
        r = refs[s].filter_cloud(clouds[s], tuple(origins[s]), float(base_z[s]))
        assert np.array_equal(labels[b, : len(clouds[s])], r["label"]), s
    assert_export_equals(planes, seg, rest, ["ground", "groundpatch"], lambda s: {k: refs[s].layer(k) for k in ("ground", "groundpatch")},
                         "after the fresh batch")
    seg.close()


# ---------------------------------------------------------------- 4. the lazily kept layers

@pytest.mark.parametrize("eager", [False, True])
def test_lazy_layers(eager):
    import torch

    slots = [4, 1, 5, 2, 0]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    if eager:
        seg.set_flags(eager_layers=True)
    for s in slots:
        seg.map(s).reset()
    refs = {s: oracle.OracleMap(120.0, 0.33) for s in slots}
    warm_maps(seg, slots, seed=1600, frames=2, refs=[refs[s] for s in slots])
    want = {s: {k: refs[s].layer(k) for k in LAYERS} for s in slots}
    subset = [5, 4, 0]
    first = seg.export_layers(LAZY, slots=subset)
    second = seg.export_layers(LAZY, slots=subset, row_major=True)
    torch.cuda.synchronize()
    assert_export_equals(first.cpu().numpy(), seg, subset, LAZY, lambda s: want[s], "first export")
    assert_export_equals(second.cpu().numpy(), seg, subset, LAZY, lambda s: want[s], "second export", row_major=True)
    for s in slots:  # the getter afterwards: the exported slots, and those it still has to compute them for
        got = seg.map(s).layers()
        for name in LAYERS:
            assert same_bits(got[name], want[s][name]), (s, name)
    everything = seg.export_layers(slots=slots)
    torch.cuda.synchronize()
    assert_export_equals(everything.cpu().numpy(), seg, slots, list(LAYERS), lambda s: want[s], "all eleven")
    seg.close()


# ---------------------------------------------------------------- 5. ordering

@pytest.mark.parametrize("halves", [False, True])
def test_export_between_two_batches_on_another_stream(halves):
    import torch

    n_slots, slots = 16, [2, 9, 5, 12, 7, 8, 15, 0]  # both halves (boundary 8)
    K = len(slots)
    base = [synth.hdl64_cloud(seed=1700 + k, n_az=200) for k in range(K)]
    stride = stride_of(base)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride) for _ in range(2)]
    if halves:
        segs[0].set_flags(concurrent_halves=True)
        segs[0].debug_set_tuning("halves_min_clouds", 2)
    for seg in segs:
        seg.reset_maps(odom_z=0.0)
        seg.synchronize()
    pts = [batch_points(base, stride), batch_points(base[::-1], stride)]
    n_pts = [[len(c) for c in base], [len(c) for c in base[::-1]]]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    odoms = np.array([(1.1 * (1 + k % 3), -0.8 * (k % 2)) for k in range(K)])
    torch.cuda.synchronize()  # (the uploads ran on torch's default stream)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        segs[0].filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
    planes = segs[0].export_layers(slots=slots, stream=b.cuda_stream)  # no synchronisation in between: the library orders it
    with torch.cuda.stream(a):
        segs[0].move_maps(odoms, [POSE] * K, slots=slots, on_torch_stream=True)
        segs[0].filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    planes = planes.cpu().numpy()
    # the same sequence on the other context, one step at a time
    segs[1].filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    between = {s: segs[1].map(s).layers() for s in slots}
    assert_export_equals(planes, segs[0], slots, list(LAYERS), lambda s: between[s], "the state between the two batches")
    segs[1].move_maps(odoms, [POSE] * K, slots=slots, on_torch_stream=True)
    segs[1].filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    for s in range(n_slots):  # ... and the second batch ran on what the first one left, not on anything the export disturbed
        got, want = segs[0].map(s).layers(), segs[1].map(s).layers()
        for name in LAYERS:
            assert same_bits(got[name], want[name]), (s, name)
    for seg in segs:
        seg.close()


def test_torch_op_right_behind_the_export():
    import torch

    slots = [1, 3, 0]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.reset_maps(odom_z=0.2)
    warm_maps(seg, slots, seed=1800, frames=2)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = torch.zeros((3, 2, seg.cols, seg.rows), dtype=torch.float32, device="cuda")
        planes = seg.export_layers(["ground", "groundpatch"], slots=slots, out=out)
        doubled = planes * 2.0  # (same stream, no synchronise in between)
        copy = planes.clone()
    stream.synchronize()
    copy, doubled = copy.cpu().numpy(), doubled.cpu().numpy()
    want = {s: seg.map(s).layers(["ground", "groundpatch"]) for s in slots}
    assert_export_equals(copy, seg, slots, ["ground", "groundpatch"], lambda s: want[s], "clone behind the export")
    assert_export_equals(doubled, seg, slots, ["ground", "groundpatch"], lambda s: {k: v * np.float32(2.0) for k, v in want[s].items()}, "2 x planes")
    seg.close()


# ---------------------------------------------------------------- 6. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    seg.reset_maps(odom_z=0.4)
    warm_maps(seg, [4, 1], seed=1900, frames=1)
    C_ = seg.rows * seg.cols
    names = ["ground", "groundpatch", "planeDist"]
    mask = mask_of(names)
    before = seg.export_layers(names)
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    dst = sentinel_tensor(2 * 3 * C_)
    p = dst.data_ptr()
    INVALID, CAPACITY = -1, -5
    col = _lib.GG_PLANES_COLMAJOR
    assert seg._L.gg_export_layers(None, 2, None, 0, mask, col, C.c_void_p(p), C_, None) == INVALID
    assert raw_export(seg, -1, None, 0, mask, col, p, C_) == INVALID
    assert raw_export(seg, 2, [1, 1], 0, mask, col, p, C_) == INVALID
    assert raw_export(seg, 2, None, 0, mask | (1 << _lib.GG_NUM_LAYERS), col, p, C_) == INVALID
    assert raw_export(seg, 2, None, 0, 0, col, p, C_) == INVALID
    assert raw_export(seg, 2, None, 0, mask, 2, p, C_) == INVALID
    assert raw_export(seg, 2, None, 0, mask, -1, p, C_) == INVALID
    assert raw_export(seg, 2, None, 0, mask, col, None, C_) == INVALID
    assert raw_export(seg, 2, None, 0, mask, col, p, C_ - 1) == INVALID
    assert raw_export(seg, 2, [1, 6], 0, mask, col, p, C_) == CAPACITY
    assert raw_export(seg, 2, [-1, 2], 0, mask, col, p, C_) == CAPACITY
    assert raw_export(seg, 2, None, 5, mask, col, p, C_) == CAPACITY
    assert raw_export(seg, 2, None, -1, mask, col, p, C_) == CAPACITY
    assert raw_export(seg, 0, None, 0, 0, 7, None, 0) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert np.all(dst.cpu().numpy().view(np.uint32) == SENTINEL)
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(names)
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    want = {s: seg.map(s).layers(names) for s in range(6)}
    assert_export_equals(after.cpu().numpy(), seg, list(range(6)), names, lambda s: want[s], "after the errors")
    seg.close()


# ---------------------------------------------------------------- 7. per-map configurations

def test_per_map_configurations():
    import torch

    slots = [2, 0]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=3, max_points=20000)
    cfgs = [api.default_config(), api.default_config()]
    cfgs[0].occupied_cells_decrease_factor = 1.1
    cfgs[1].occupied_cells_decrease_factor = 3.0
    seg.set_slot_configs(cfgs, slots=slots)
    refs = []
    for c in cfgs:
        r = oracle.OracleMap(120.0, 0.33)
        o = oracle.default_config()
        for name, _ in _lib.GGConfig._fields_:
            setattr(o, name, getattr(c, name))
        r.cfg = o
        refs.append(r)
    for s in slots:
        seg.map(s).reset()
    # the same clouds for both maps: whatever differs comes from the configuration
    base = [synth.hdl64_cloud(seed=2000 + f, n_az=260) for f in range(3)]
    stride = stride_of(base)
    for f, c in enumerate(base):
        seg.filter_batch(batch_points([c, c], stride), [len(c)] * 2, np.zeros((2, 3), np.float32), np.full(2, -1.73), slots=slots)
        torch.cuda.synchronize()
        for r in refs:
            r.filter_cloud(c, (0.0, 0.0, 0.0), -1.73)
    planes = seg.export_layers(["ground", "groundpatch"], slots=slots)
    torch.cuda.synchronize()
    planes = planes.cpu().numpy()
    assert not same_bits(planes[0, 1], planes[1, 1])
    for i in range(2):
        assert_export_equals(planes[i: i + 1], seg, [slots[i]], ["ground", "groundpatch"],
                             lambda s: {k: refs[i].layer(k) for k in ("ground", "groundpatch")}, f"configuration {i}")
    seg.close()
