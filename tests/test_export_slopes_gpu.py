"""gg_export_slopes (slope, step and normal planes of many maps, one launch) on the device, held to the definition of
include/groundgrid_hip.h in its numpy form (tests/slopes_ref.py).  Every comparison is on bits, except that a cell of grad_x, grad_y,
tangent or normal_z whose reference value is NaN must only be NaN on the device too (which NaN is not specified).  Shapes: 79 x 79 (two
blocks per axis, 64 + 15: the halo crosses a block seam, the last block is narrow, all four clamped borders and corners are in play) and
364 x 364 (six blocks per axis, the last 44 wide)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402
from groundgrid_amd._lib import LAYERS, SLOPE_CHANNELS  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.slopes_ref import FRESH, slopes_reference  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # (a NaN payload nothing produces)
POSE = (0.3, 0.2, 1.5, 0.02, -0.01, 0.3, 0.95)
PARAM_RING = 4  # (gg_context.hip: entries of a call's parameter ring)
GEOMETRY = {79: (26.0, 0.33), 364: (120.0, 0.33)}
ALL = (1 << _lib.GG_NUM_SLOPE_CHANNELS) - 1
COL, ROW = _lib.GG_PLANES_COLMAJOR, _lib.GG_PLANES_ROWMAJOR
INVALID, CAPACITY = -1, -5


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


def fresh_count(seg):
    return seg.debug_set_tuning("fresh_count", 0)


def lazy_count(seg):
    return seg.debug_set_tuning("lazy_count", 0)


def sentinel_tensor(count):
    import torch

    return torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def mask_of(names):
    return sum(1 << SLOPE_CHANNELS.index(k) for k in names)


def names_of(mask):
    return [k for i, k in enumerate(SLOPE_CHANNELS) if (mask >> i) & 1]


def raw_slopes(seg, n, slots, first_slot, mask, order, dst_ptr, plane_stride, stream=None):
    """gg_export_slopes as the C ABI has it; returns the status"""
    import torch

    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_export_slopes(seg._ctx, n, sl, first_slot, mask, order, C.c_void_p(dst_ptr) if dst_ptr else None, plane_stride,
                                   C.c_void_p(s if s else _lib.GG_STREAM_DEFAULT))


def warm_maps(seg, slots, seed, frames=2, n_az=150, refs=None):
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


def assert_channel(got, want, channel, tag):
    """got, want: (rows, cols) planes of one channel"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, tag
    free = np.zeros(want.shape, bool)
    if SLOPE_CHANNELS.index(channel) < 4:
        free = np.isnan(want)
        assert np.all(np.isnan(got[free])), f"{tag}: {channel}: {int((~np.isnan(got[free])).sum())} cells are not NaN where the definition is"
    bad = (bits(got) != bits(want)) & ~free
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: {channel}: {int(bad.sum())} cells differ, first at ({r}, {c}): got {got[r, c]!r} ({bits(got)[r, c]:#x}), "
                             f"want {want[r, c]!r} ({bits(want)[r, c]:#x})")


def assert_slopes(planes, names, want_of, slots, row_major, tag):
    """planes: what export_slopes returned, on the host; want_of(slot) -> the six reference planes"""
    for i, s in enumerate(slots):
        want = want_of(s)
        for k, name in enumerate(names):
            got = planes[i, k] if row_major else planes[i, k].T
            assert_channel(got, want[SLOPE_CHANNELS.index(name)], name, f"{tag}: map {i} (slot {s})")


def plane_of(flat, rows, cols, at, order):
    p = flat[at: at + rows * cols]
    return p.reshape(rows, cols) if order == ROW else p.reshape((rows, cols), order="F")


# ---------------------------------------------------------------- 1. parity with the oracle; 6. the cell-by-cell form

@pytest.fixture(scope="module", params=[79, 364])
def scene(request):
    """a context whose maps are warm and scrolled (4, 1), warm (3) and fresh (0, 2, 5), with the oracle's (ground, groundpatch) per slot"""
    import torch

    size = request.param
    length, res = GEOMETRY[size]
    seg = api.GroundSegmentation().init(length, res, n_slots=6, max_points=20000)
    assert seg.rows == seg.cols == size
    seg.reset_maps(odom_z=0.3)
    refs = {s: oracle.OracleMap(length, res, odom_z=0.3) for s in range(6)}
    warm_maps(seg, [4, 1], seed=5100, frames=2, refs=[refs[4], refs[1]])
    warm_maps(seg, [3], seed=5200, frames=1, refs=[refs[3]])
    torch.cuda.synchronize()
    assert fresh_count(seg) == 3
    res32 = np.float32(seg.resolution)
    pairs = {s: (refs[s].layer("ground"), refs[s].layer("groundpatch")) for s in range(6)}
    want = {s: slopes_reference(pairs[s][0], pairs[s][1], res32) for s in range(6)}
    for s in (0, 2, 5):  # (a fresh map is a level plane: the definition gives the constants of the header)
        for k in range(6):
            assert np.all(bits(want[s][k]) == bits(FRESH[k]))
    sc = dict(seg=seg, size=size, res=res32, want=want, slots=[4, 0, 3, 5, 1])
    yield sc
    seg.close()


@pytest.mark.parametrize("row_major", [False, True])
def test_parity_with_the_oracle(scene, row_major):
    import torch

    seg, slots = scene["seg"], scene["slots"]
    planes = seg.export_slopes(slots=slots, row_major=row_major)
    layers = seg.export_layers(["ground", "groundpatch"], slots=slots, row_major=True)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 3
    assert planes.shape == ((len(slots), 6, seg.rows, seg.cols) if row_major else (len(slots), 6, seg.cols, seg.rows))
    planes, layers = planes.cpu().numpy(), layers.cpu().numpy()
    tag = f"{scene['size']} {'row' if row_major else 'col'}-major"
    assert_slopes(planes, SLOPE_CHANNELS, lambda s: scene["want"][s], slots, row_major, tag + " against the oracle")
    exported = {s: slopes_reference(layers[i, 0], layers[i, 1], scene["res"]) for i, s in enumerate(slots)}
    assert_slopes(planes, SLOPE_CHANNELS, lambda s: exported[s], slots, row_major, tag + " against export_layers")
    # the maps are terrain, not constants: the comparison above has something to compare
    i = slots.index(4)
    step = planes[i, 4]
    assert np.count_nonzero(step) > step.size // 10 and not np.isnan(step).any() and not np.signbit(step).any()


@pytest.mark.parametrize("row_major", [False, True])
def test_cell_by_cell_form_gives_the_same_bits(scene, row_major):
    import torch

    seg, slots = scene["seg"], scene["slots"]
    tiled = seg.export_slopes(slots=slots, row_major=row_major)
    try:
        assert seg.debug_set_tuning("slopes_variant", 1) == 0
        gathered = seg.export_slopes(slots=slots, row_major=row_major)
        subset = seg.export_slopes(["grad_y", "step"], slots=slots, row_major=row_major)
    finally:
        seg.debug_set_tuning("slopes_variant", 0)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 3
    tiled, gathered, subset = tiled.cpu().numpy(), gathered.cpu().numpy(), subset.cpu().numpy()
    assert same_bits(tiled, gathered), f"{int((bits(tiled) != bits(gathered)).sum())} cells differ"
    assert same_bits(tiled[:, [1, 4]], subset)
    assert_slopes(gathered, SLOPE_CHANNELS, lambda s: scene["want"][s], slots, row_major, f"{scene['size']} cell by cell")


# ---------------------------------------------------------------- 2. engineered planes through import_layers; 3. channel subsets

def engineered_planes(n, res):
    """(ground, groundpatch) pairs of n x n cells that aim at the kernel's seams, borders and the definition's special values"""
    rng = np.random.default_rng(77)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    conf = lambda: rng.uniform(0.001, 1.0, (n, n)).astype(np.float32)  # noqa: E731
    cases = {}
    # a ramp rising towards +x and falling towards +y: x = -res * row, y = -res * col
    cases["ramp"] = ((0.3 * (-res * r) - 0.7 * (-res * c) + 1.5).astype(np.float32), conf())
    cases["checkerboard"] = ((((r + c) & 1) * 0.5 - 0.25).astype(np.float32), (((r + c) & 1) * 0.5 + 0.25).astype(np.float32))
    # distinct values on the block seam (63 | 64) and on the border rows and columns
    g = rng.normal(0.0, 0.05, (n, n)).astype(np.float32)
    w = conf()
    for k, (at, axis) in enumerate([(63, 0), (64, 0), (63, 1), (64, 1), (0, 0), (n - 1, 0), (0, 1), (n - 1, 1)]):
        line = np.float32((-1) ** k * 10.0 * 2 ** k) + np.arange(n, dtype=np.float32)
        if axis == 0:
            g[at, :] += line
            w[at, :] = np.float32(2.0 ** -(k + 2))
        else:
            g[:, at] += line
            w[:, at] = np.float32(2.0 ** -(k + 12))
    cases["seams"] = (g, w)
    # +-0, +-inf, NaN, denormals and 1e30 (gx * gx overflows to inf: tangent = inf, normal_z = +0), sprinkled and at chosen places
    g = rng.normal(0.0, 0.2, (n, n)).astype(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-45, 1e30, -1e30], dtype=np.float32)
    pick = rng.random((n, n)) < 0.08
    g[pick] = specials[rng.integers(0, len(specials), int(pick.sum()))]
    g[0, 0], g[n - 1, n - 1], g[63, 64], g[64, 63], g[0, n - 1], g[n - 1, 0] = np.nan, np.inf, -np.inf, 1e30, -0.0, 1e-40
    g[20:23, 30] = (np.float32(1e30), np.float32(0.25), np.float32(-1e30))  # an overflowing gradient with a finite centre
    g[19:24, 29], g[19:24, 31] = 0.5, 0.5
    g[40:43, 40:43] = np.float32(1e-40) * np.arange(9, dtype=np.float32).reshape(3, 3)  # a neighbourhood of denormals
    g[50:53, 50:53] = 0.0
    g[51, 51] = -0.0
    cases["specials"] = (g, conf())
    # NaN confidence in some cells of a neighbourhood ...
    w = conf()
    w[rng.random((n, n)) < 0.3] = np.nan
    cases["some NaN confidence"] = (rng.normal(0.0, 0.1, (n, n)).astype(np.float32), w)
    # ... and in all of them: blocks across the seam, in a corner and along a border
    w = conf()
    w[60:68, 60:68] = np.nan
    w[0:4, 0:4] = np.nan
    w[n - 3:, 10:40] = np.nan
    w[30:33, 30:33] = np.nan  # (exactly one neighbourhood: only its centre is NaN)
    w[10, 10] = np.inf
    w[12, 12] = 1e-42
    cases["all NaN confidence"] = (rng.normal(0.0, 0.1, (n, n)).astype(np.float32), w)
    return cases


@pytest.fixture(scope="module")
def engineered():
    import torch

    length, res = GEOMETRY[79]
    seg = api.GroundSegmentation().init(length, res, n_slots=7, max_points=4096)
    res32 = np.float32(seg.resolution)
    cases = engineered_planes(seg.rows, float(res32))
    names = list(cases)
    seg.reset_maps(odom_z=0.3)
    src = np.stack([np.stack(cases[k]) for k in names])  # [6, 2, rows, cols]
    seg.import_layers(torch.from_numpy(src).cuda(), ["ground", "groundpatch"], first_slot=0, n=len(names), row_major=True)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 1  # (slot 6)
    want = {i: slopes_reference(cases[k][0], cases[k][1], res32) for i, k in enumerate(names)}
    want[6] = [np.full((seg.rows, seg.cols), v, np.float32) for v in FRESH]
    yield dict(seg=seg, names=names, cases=cases, want=want, res=res32)
    seg.close()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("row_major", [False, True])
def test_engineered_planes(engineered, row_major, variant):
    import torch

    seg, want = engineered["seg"], engineered["want"]
    slots = [5, 2, 6, 0, 4, 1, 3]
    try:
        seg.debug_set_tuning("slopes_variant", variant)
        planes = seg.export_slopes(slots=slots, row_major=row_major)
    finally:
        seg.debug_set_tuning("slopes_variant", 0)
    torch.cuda.synchronize()
    planes = planes.cpu().numpy()
    for i, s in enumerate(slots):
        tag = f"{engineered['names'][s] if s < 6 else 'fresh'}, {'row' if row_major else 'col'}-major, variant {variant}"
        assert_slopes(planes[i: i + 1], SLOPE_CHANNELS, lambda s: want[s], [s], row_major, tag)
    # the cases hold what they were built for
    ramp = want[engineered["names"].index("ramp")]
    assert np.allclose(ramp[0], 0.3, rtol=0, atol=5e-5) and np.allclose(ramp[1], -0.7, rtol=0, atol=5e-5)  # dz/dx > 0, dz/dy < 0
    sp = want[engineered["names"].index("specials")]
    assert np.isfinite(sp[0][21, 30]) and np.isinf(sp[2][21, 30]) and bits(sp[3])[21, 30] == 0  # gx * gx overflows: tangent inf, normal_z +0
    assert np.isnan(sp[0]).any() and not np.isnan(sp[4]).any() and not np.signbit(sp[4]).any()
    assert np.any((sp[4] > 0) & (sp[4] < 1e-38))  # a denormal step
    nanw = want[engineered["names"].index("all NaN confidence")][5]
    assert np.isnan(nanw[62:66, 62:66]).all() and np.isnan(nanw[0, 0]) and np.isnan(nanw[78, 20]) and np.isnan(nanw[31, 31])
    assert int(np.isnan(nanw[29:34, 29:34]).sum()) == 1 and nanw[10, 10] < 1.0 and nanw[11, 11] == np.float32(1e-42)


@pytest.mark.parametrize("order", [COL, ROW])
def test_channel_subsets_write_nothing_else(engineered, order):
    import torch

    seg, want = engineered["seg"], engineered["want"]
    rows, cols = seg.rows, seg.cols
    C_ = rows * cols
    stride = C_ + 38
    assert stride % 2 == 1
    slots, guard = [2, 6, 3], 3  # (a destination that is 4-byte aligned and no more)
    masks = [1 << k for k in range(6)] + [mask_of(["tangent", "step"]), ALL]
    dsts = []
    for m in masks:
        K = bin(m).count("1")
        dst = sentinel_tensor(guard + len(slots) * K * stride + guard)
        assert (dst.data_ptr() + 4 * guard) % 8 == 4
        assert raw_slopes(seg, len(slots), slots, 0, m, order, dst.data_ptr() + 4 * guard, stride) == 0, seg._L.gg_last_error(seg._ctx)
        dsts.append(dst)
    torch.cuda.synchronize()
    for m, dst in zip(masks, dsts):
        flat = dst.cpu().numpy()
        names = names_of(m)
        K = len(names)
        written = np.zeros(flat.shape, bool)
        for i, s in enumerate(slots):
            for k, name in enumerate(names):
                at = guard + (i * K + k) * stride
                assert_channel(plane_of(flat, rows, cols, at, order), want[s][SLOPE_CHANNELS.index(name)], name, f"mask {m:#b}, map {i}")
                written[at: at + C_] = True
        assert np.all(flat.view(np.uint32)[~written] == SENTINEL), f"mask {m:#b}: something outside the named planes was written"
        assert int((~written).sum()) == 2 * guard + len(slots) * K * (stride - C_)


def test_python_entry_point(engineered):
    import torch

    seg, want = engineered["seg"], engineered["want"]
    C_ = seg.rows * seg.cols
    a = seg.export_slopes()
    assert a.shape == (7, 6, seg.cols, seg.rows) and a.dtype == torch.float32 and a.is_cuda
    b = seg.export_slopes(["tangent", "step"], slots=[3, 0], row_major=True)
    assert b.shape == (2, 2, seg.rows, seg.cols)
    out = torch.zeros((2, 1, seg.cols, seg.rows), dtype=torch.float32, device="cuda")
    assert seg.export_slopes(["min_confidence"], first_slot=5, n=2, out=out) is out
    flat = seg.export_slopes(["grad_x"], slots=[1], plane_stride=C_ + 5)
    assert flat.shape == (C_ + 5,)
    for bad in (["step", "tangent"], ["step", "step"], ["slope"], []):
        with pytest.raises(ValueError):
            seg.export_slopes(bad)
    torch.cuda.synchronize()
    assert_slopes(a.cpu().numpy(), SLOPE_CHANNELS, lambda s: want[s], list(range(7)), False, "all")
    assert_slopes(b.cpu().numpy(), ["tangent", "step"], lambda s: want[s], [3, 0], True, "row-major subset")
    assert_slopes(out.cpu().numpy(), ["min_confidence"], lambda s: want[s], [5, 6], False, "out")
    assert_channel(plane_of(flat.cpu().numpy(), seg.rows, seg.cols, 0, COL), want[1][0], "grad_x", "plane_stride")


# ---------------------------------------------------------------- 4. fresh maps

def test_fresh_maps_get_the_constants_and_stay_fresh():
    import torch

    B = 100
    clouds = [synth.hdl64_cloud(seed=5500 + k, n_az=96 + (k % 5) * 3) for k in range(B)]
    stride = stride_of(clouds)
    pts = batch_points(clouds, stride)
    n_pts = [len(c) for c in clouds]
    origins = np.array([[0.05 * (b % 7), -0.03 * (b % 5), 0.01 * (b % 3)] for b in range(B)], dtype=np.float32)
    base_z = np.array([-1.73 + 0.003 * (b % 9) for b in range(B)])
    want = torch.from_numpy(np.array([int(bits(v)[0]) for v in FRESH], dtype=np.int32)).cuda()
    results = []
    for which in range(2):
        seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
        seg.reset_maps(0, 50, odom_z=0.25, on_torch_stream=True)
        seg.reset_maps(50, 50, odom_z=-1.5, on_torch_stream=True)
        assert fresh_count(seg) == B
        if which == 0:
            out = None
            for row_major, variant in ((False, 0), (True, 0), (False, 1), (True, 1)):
                seg.debug_set_tuning("slopes_variant", variant)
                out = seg.export_slopes(row_major=row_major, out=out)  # (rows == cols: one shape)
                equal = (out.view(torch.int32).view(B, 6, -1) == want[None, :, None]).all().item()  # (on bits, on the device)
                assert equal, f"row_major {row_major}, variant {variant}"
                assert fresh_count(seg) == B
            seg.debug_set_tuning("slopes_variant", 0)
            sub = seg.export_slopes(["normal_z", "min_confidence"], slots=[99, 0, 50])
            assert (sub.view(torch.int32).view(3, 2, -1) == want[[3, 5]][None, :, None]).all().item()
            assert fresh_count(seg) == B
        # the batch behind it: what a context that never made the call gives
        batch = seg.filter_batch(pts, n_pts, origins, base_z)
        assert fresh_count(seg) == 0
        planes = seg.export_layers(["ground", "groundpatch"], first_slot=0, n=B)
        torch.cuda.synchronize()
        results.append((batch.labels.cpu().numpy(), batch.counts.cpu().numpy(), planes.cpu().numpy()))
        seg.close()
    a, b = results
    assert np.array_equal(a[1], b[1])
    for k in range(B):
        assert np.array_equal(a[0][k, : n_pts[k]], b[0][k, : n_pts[k]]), k
    assert same_bits(a[2], b[2])


# ---------------------------------------------------------------- 5. twin contexts: nothing changes

def test_nothing_changes():
    import torch

    slots = [4, 1, 5, 2]
    K = len(slots)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000) for _ in range(2)]
    base = [synth.hdl64_cloud(seed=5600 + k, n_az=150 + 7 * k) for k in range(K)]
    stride = stride_of(base)
    pts = [batch_points(base, stride), batch_points(base[::-1], stride)]
    n_pts = [[len(c) for c in base], [len(c) for c in base[::-1]]]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    lazy = ["maxGroundHeight", "groundCandidates", "planeDist"]
    results = []
    for which, seg in enumerate(segs):
        seg.reset_maps(odom_z=0.1)
        seg.set_scoring(slots=slots)
        seg.filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
        assert lazy_count(seg) == K
        if which == 0:  # the call between the two batches, on every map of the context (two of them fresh), in every form
            for variant in (0, 1):
                seg.debug_set_tuning("slopes_variant", variant)
                for row_major in (False, True):
                    slopes = seg.export_slopes(row_major=row_major)
                seg.export_slopes(["step"], slots=slots)
            seg.debug_set_tuning("slopes_variant", 0)
        # the lazily kept layers are still owed behind the call: their first reader computes them, to the values of the twin
        assert lazy_count(seg) == K
        pending = seg.export_layers(lazy, slots=slots)
        assert lazy_count(seg) == 0
        second = seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
        planes = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:
            assert np.count_nonzero(slopes[4, 4].cpu().numpy()) > 1000  # (the call had terrain in front of it)
        results.append(dict(fresh=fresh_count(seg), pending=pending.cpu().numpy(), planes=planes.cpu().numpy(), labels=second.labels.cpu().numpy(),
                            index=second.out_index.cpu().numpy(), counts=second.counts.cpu().numpy(), scores=seg.scores_raw(),
                            positions=[seg.map(s).getPosition() for s in range(6)]))
    a, b = results
    assert a["fresh"] == b["fresh"] == 2
    assert same_bits(a["pending"], b["pending"]) and same_bits(a["planes"], b["planes"])
    assert a["planes"].shape[1] == len(LAYERS) == 11
    assert np.array_equal(a["counts"], b["counts"]) and a["positions"] == b["positions"]
    for k in range(K):
        assert np.array_equal(a["labels"][k, : n_pts[1][k]], b["labels"][k, : n_pts[1][k]]) and np.array_equal(a["index"][k, : n_pts[1][k]], b["index"][k, : n_pts[1][k]])
    assert np.array_equal(a["scores"][0], b["scores"][0]) and np.array_equal(a["scores"][1], b["scores"][1]) and a["scores"][0].sum() == 2 * K
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 7. a caller's stream, past the ring, no host synchronisation

@pytest.mark.parametrize("halves", [False, True])
def test_rounds_on_a_caller_stream(halves):
    import torch

    n_slots, slots = 4, [2, 1, 3, 0]  # both halves (boundary 2)
    K, rounds, moved_at = len(slots), PARAM_RING + 2, 3
    base = [synth.hdl64_cloud(seed=5700 + k, n_az=60 + 5 * k) for k in range(K)]
    stride = stride_of(base)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride)
    if halves:
        seg.set_flags(concurrent_halves=True)
        seg.debug_set_tuning("halves_min_clouds", 2)
    odoms = np.array([(0.9 * (1 + k % 3), -0.7 * (k % 2)) for k in range(K)])
    sets, origins = [], []
    for r in range(rounds):
        cs = [synth.clone_cloud(c) for c in (base if r % 2 == 0 else base[::-1])]
        at = odoms if r >= moved_at else np.zeros((K, 2))
        for k, c in enumerate(cs):
            c["x"] += np.float32(at[k][0])
            c["y"] += np.float32(at[k][1])
        sets.append(cs)
        origins.append(np.array([(at[k][0], at[k][1], 0.0) for k in range(K)], dtype=np.float32))
    pts = [batch_points(cs, stride) for cs in sets]
    n_pts = [[len(c) for c in cs] for cs in sets]
    base_z = np.full(K, -1.73)
    C_ = seg.rows * seg.cols
    plane_stride = C_ + 3
    dsts = [sentinel_tensor(K * 6 * plane_stride) for _ in range(rounds)]
    torch.cuda.synchronize()  # (the uploads and the fills ran on torch's default stream)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        for r in range(rounds):  # no synchronisation anywhere: every call has its own planes
            if r == moved_at:
                seg.move_maps(odoms, [POSE] * K, slots=slots, on_torch_stream=True)
            seg.filter_batch(pts[r], n_pts[r], origins[r], base_z, slots=slots)
            order = ROW if r % 2 else COL
            assert raw_slopes(seg, K, slots, 0, ALL, order, dsts[r].data_ptr(), plane_stride) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    res32 = np.float32(seg.resolution)
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    for r in range(rounds):
        flat = dsts[r].cpu().numpy()
        order = ROW if r % 2 else COL
        for i in range(K):
            if r == moved_at:
                refs[i].update(odoms[i][0], odoms[i][1], POSE)
            refs[i].filter_cloud(sets[r][i], tuple(origins[r][i]), -1.73)
            want = slopes_reference(refs[i].layer("ground"), refs[i].layer("groundpatch"), res32)
            for k, name in enumerate(SLOPE_CHANNELS):
                at = (i * 6 + k) * plane_stride
                assert_channel(plane_of(flat, seg.rows, seg.cols, at, order), want[k], name, f"round {r}, halves {halves}, map {i}")
                assert np.all(flat.view(np.uint32)[at + C_: at + plane_stride] == SENTINEL)
    seg.close()


# ---------------------------------------------------------------- 8. errors change nothing

def test_errors_change_nothing():
    import torch

    length, res = GEOMETRY[79]
    seg = api.GroundSegmentation().init(length, res, n_slots=6, max_points=20000)
    seg.reset_maps(odom_z=0.4)
    warm_maps(seg, [4, 1], seed=5900, frames=1)
    C_ = seg.rows * seg.cols
    before = seg.export_slopes()
    layers_before = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)
    assert fresh_before == 4 and lazy_before == 2
    dst = sentinel_tensor(2 * 6 * C_)
    p = dst.data_ptr()
    errors = [
        (lambda: seg._L.gg_export_slopes(None, 2, None, 0, ALL, COL, C.c_void_p(p), C_, None), INVALID),
        (lambda: raw_slopes(seg, -1, None, 0, ALL, COL, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, [1, 1], 0, ALL, COL, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL | (1 << _lib.GG_NUM_SLOPE_CHANNELS), COL, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, 1 << 31, COL, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, 0, COL, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL, 2, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL, -1, p, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL, COL, None, C_), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL, COL, p, C_ - 1), INVALID),
        (lambda: raw_slopes(seg, 2, None, 0, ALL, COL, p, 0), INVALID),
        (lambda: raw_slopes(seg, 2, [1, 6], 0, ALL, COL, p, C_), CAPACITY),
        (lambda: raw_slopes(seg, 2, [-1, 2], 0, ALL, COL, p, C_), CAPACITY),
        (lambda: raw_slopes(seg, 2, None, 5, ALL, COL, p, C_), CAPACITY),
        (lambda: raw_slopes(seg, 2, None, -1, ALL, COL, p, C_), CAPACITY),
    ]
    for k, (call, code) in enumerate(errors):
        assert call() == code, k
        torch.cuda.synchronize()
        assert bool((dst.view(torch.int32) == SENTINEL).all().item()), f"error {k} wrote to the destination"
        assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before, k
        # a valid call right behind it is correct
        after = seg.export_slopes(row_major=bool(k % 2))
        torch.cuda.synchronize()
        after = after if k % 2 == 0 else after.transpose(2, 3).contiguous()
        assert bool((after.view(torch.int32) == before.view(torch.int32)).all().item()), f"the call behind error {k}"
    assert raw_slopes(seg, 0, None, 0, 0, 7, None, 0) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert np.all(dst.cpu().numpy().view(np.uint32) == SENTINEL)
    layers_after = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    assert same_bits(layers_before.cpu().numpy(), layers_after.cpu().numpy())
    res32 = np.float32(seg.resolution)
    host, layers = before.cpu().numpy(), layers_before.cpu().numpy()
    want = {s: slopes_reference(layers[s, 0].T, layers[s, 1].T, res32) for s in range(6)}
    assert_slopes(host, SLOPE_CHANNELS, lambda s: want[s], list(range(6)), False, "the valid call")
    seg.close()
