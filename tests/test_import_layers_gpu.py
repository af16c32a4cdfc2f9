"""gg_import_layers (dense planes in device memory into the layers of many maps, one launch) on the device: bit for bit what gg_set_layer
leaves per map and layer, the round trip with gg_export_layers, a restored map that continues like the original and like the CPU oracle,
fresh maps, the lazily kept layers, the sparse per-call layers, caller streams, and errors that change nothing.  Every comparison is on
bits; there is no tolerance."""
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
from tests import test_export_layers_gpu as ex  # noqa: E402  (its helpers: the two entry points are tested the same way)

pytestmark = pytest.mark.gpu

LAZY = ["maxGroundHeight", "groundCandidates", "planeDist"]
PERCALL = [k for k in LAYERS if k not in ("ground", "groundpatch")]
# (the first mask with a per-call layer names ONE of the three lazily kept ones while they are still pending)
MASKS = [["ground"], ["groundpatch"], ["ground", "groundpatch"], ["planeDist"], LAZY, ["points", "minGroundHeight", "m2", "pointsRaw", "variance"],
         list(LAYERS)]
SENTINEL = ex.SENTINEL  # (a NaN payload no layer and no source plane holds)
VARIANTS = [0, 1]       # 0: k_import_tiled, 1: the batched materialise + k_import_scatter
FLT_MAX, FLT_MIN = np.float32(3.402823466e+38), np.float32(1.175494351e-38)
bits, same_bits, batch_points, stride_of, mask_of, fresh_count = ex.bits, ex.same_bits, ex.batch_points, ex.stride_of, ex.mask_of, ex.fresh_count


def ibits(t):
    import torch

    return t.contiguous().view(torch.int32)


def same_on_device(a, b):
    import torch

    return torch.equal(ibits(a), ibits(b))


def random_pool(count, seed, finite=False):
    """`count` floats on both sides of 0.01, with a NaN that carries a payload, both infinities, -0.0 and denormals sprinkled in
    (finite: without the NaNs and infinities -- for terrain that a sweep then computes with and the CPU oracle is compared to on bits:
    which payload a NaN has after arithmetic is the processor's business)"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(count) * 0.02).astype(np.float32)
    special = np.array([0x7FC0BEEF, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00000000], dtype=np.uint32).view(np.float32)
    at = rng.choice(count, size=max(8, count // 97), replace=False)
    v[at] = special[np.arange(at.size) % special.size]
    if finite:
        v[~np.isfinite(v)] = np.float32(0.011)
    assert not np.any(v.view(np.uint32) == SENTINEL)
    return v


def raw_import(seg, n, slots, first_slot, mask, order, src_ptr, plane_stride, stream=None):
    """gg_import_layers as the C ABI has it; returns the status"""
    import torch

    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_import_layers(seg._ctx, n, sl, first_slot, mask, order, C.c_void_p(src_ptr) if src_ptr else None, plane_stride,
                                   C.c_void_p(s if s else _lib.GG_STREAM_DEFAULT))


def host_planes(flat, seg, n, K, stride, row_major):
    """the (rows, cols) arrays of a downloaded source: [map][plane]"""
    return [[ex.plane_of(flat, seg, i, K, k, stride, row_major) for k in range(K)] for i in range(n)]


def frame_clouds(base, f, K):
    odoms = np.array([(0.9 * f * (1 + k % 3), -0.7 * f * (k % 2)) for k in range(K)])
    clouds = []
    for k in range(K):
        c = synth.clone_cloud(base[(k + f) % K])
        c["x"] += np.float32(odoms[k][0])
        c["y"] += np.float32(odoms[k][1])
        clouds.append(c)
    origins = np.array([(odoms[k][0], odoms[k][1], 0.0) for k in range(K)], dtype=np.float32)
    return odoms, clouds, origins


def run_frames(seg, slots, base, frames, refs=None, move_first=True):
    """frames (ex.warm_maps' recipe: a scroll in front of every frame but frame 0, then a batch); returns the batches' outputs on the host,
    and the oracle's when `refs` run along"""
    import torch

    K, stride, outs, wants = len(slots), stride_of(base), [], []
    for f in frames:
        odoms, clouds, origins = frame_clouds(base, f, K)
        if f and move_first:
            seg.move_maps(odoms, [ex.POSE] * K, slots=slots, on_torch_stream=True)
        o = seg.filter_batch(batch_points(clouds, stride), [len(c) for c in clouds], origins, np.full(K, -1.73), slots=slots)
        torch.cuda.synchronize()
        outs.append((o.labels.cpu().numpy(), o.out_index.cpu().numpy(), o.counts.cpu().numpy(), [len(c) for c in clouds]))
        if refs is not None:
            w = []
            for k in range(K):
                if f:
                    refs[k].update(odoms[k][0], odoms[k][1], ex.POSE)
                w.append(refs[k].filter_cloud(clouds[k], tuple(origins[k]), -1.73))
            wants.append(w)
    return outs, wants


def assert_same_outputs(a, b, tag):
    for f, ((la, ia, ca, n), (lb, ib, cb, _)) in enumerate(zip(a, b)):
        assert np.array_equal(ca, cb), f"{tag}: counts of frame {f}"
        for k, nk in enumerate(n):
            assert np.array_equal(la[k, :nk], lb[k, :nk]), f"{tag}: labels of frame {f}, cloud {k}"
            assert np.array_equal(ia[k, :nk], ib[k, :nk]), f"{tag}: out_index of frame {f}, cloud {k}"


def assert_layers_equal_oracle(seg, slots, refs, tag, names=LAYERS):
    for s, r in zip(slots, refs):
        got = seg.map(s).layers(list(names))
        for name in names:
            assert np.array_equal(got[name], r.layer(name), equal_nan=True), f"{tag}: slot {s} layer {name}: {int((got[name] != r.layer(name)).sum())} cells differ"


# ---------------------------------------------------------------- 1. parity with gg_set_layer

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("length,res,n_slots,size", [(26.0, 0.33, 5, 79), (120.0, 0.33, 6, 364), (200.0, 0.2, 3, 1000)])
def test_parity_with_the_setter(length, res, n_slots, size, variant):
    import torch

    A, B = (api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=20000) for _ in range(2))
    assert A.rows == A.cols == size
    A.debug_set_tuning("import_variant", variant)
    written = list(range(1, n_slots))  # (slot 0 stays as the reset left it)
    for seg in (A, B):
        seg.reset_maps(odom_z=0.3)
        ex.warm_maps(seg, written, seed=2100, n_az=120)
        seg.reset_maps(n_slots - 1, 1, odom_z=0.7)  # (one map re-initialised after its clouds)
    C_ = size * size
    stride = C_ + 37
    rng = np.random.default_rng(11)
    subset = [int(s) for s in rng.permutation(n_slots)[: max(2, n_slots - 1)]]
    if 0 not in subset:
        subset[-1] = 0  # (the fresh map is in the permuted list)
    selections = [(subset, 0, len(subset)), (None, 1, n_slots - 1)]
    pool = torch.from_numpy(random_pool(n_slots * len(LAYERS) * stride + 64, seed=size + variant)).cuda()
    sentinel_seen = torch.zeros((), dtype=torch.bool, device="cuda")
    combo = 0
    fresh = {0, n_slots - 1}  # (the test's own account of which maps are fresh)
    for names in MASKS:
        for row_major in (False, True):
            for slots, first, n in selections:
                K = len(names)
                tag = f"{size} {'+'.join(names) if K < 11 else 'all'} {'row' if row_major else 'col'}-major {'list' if slots else 'range'}"
                for seg in (A, B):
                    seg.reset_maps(0, 1, odom_z=0.3)  # (slot 0 is fresh in front of every import that lists it)
                fresh.add(0)
                off = 1 + 2 * (combo % 29)  # (odd: the source is aligned to 4 bytes and no more)
                combo += 1
                src = pool[off: off + n * K * stride].clone()
                src.view(n * K, stride)[:, C_:] = ex.sentinel_tensor(1)  # (the gaps: never read, so they never reach a map)
                src = torch.cat([torch.zeros(1, device="cuda"), src])[1:]  # (data_ptr on a 4-byte boundary that is not a 16-byte one)
                assert src.data_ptr() % 16 == 4
                order = _lib.GG_PLANES_ROWMAJOR if row_major else _lib.GG_PLANES_COLMAJOR
                assert fresh_count(A) == len(fresh), tag
                assert raw_import(A, n, slots, first, mask_of(names), order, src.data_ptr(), stride) == 0, A._L.gg_last_error(A._ctx)
                listed = slots if slots is not None else list(range(first, first + n))
                if "ground" in names or "groundpatch" in names:
                    fresh -= set(listed)  # (they become real by the import alone; every other fresh map stays fresh)
                assert fresh_count(A) == len(fresh), tag
                planes = host_planes(src.cpu().numpy(), A, n, K, stride, row_major)
                for i, s in enumerate(listed):
                    for k, name in enumerate(names):
                        B.map(s).set(name, planes[i][k])
                got, want = A.export_layers(), B.export_layers()
                assert same_on_device(got, want), f"{tag}: {[(s, LAYERS[k]) for s in range(n_slots) for k in range(11) if not same_on_device(got[s, k], want[s, k])]}"
                sentinel_seen |= (ibits(got) == SENTINEL).any()
    assert not bool(sentinel_seen.item()), "a gap between two source planes reached a map"
    for s in range(n_slots):  # ... and through the host getter
        got, want = A.map(s).layers(), B.map(s).layers()
        for name in LAYERS:
            assert same_bits(got[name], want[name]), (s, name)
    # what runs on the maps afterwards sees the same state (no_confidence, the liveness marks, the lazily kept layers)
    base = [synth.hdl64_cloud(seed=2150 + k, n_az=110) for k in range(n_slots)]
    outs = [run_frames(seg, list(range(n_slots)), base, [1])[0] for seg in (A, B)]
    assert_same_outputs(outs[0], outs[1], f"{size}: a batch after the imports")
    assert same_on_device(A.export_layers(), B.export_layers())
    A.close()
    B.close()


# ---------------------------------------------------------------- 2. round trip

@pytest.mark.parametrize("variant", VARIANTS)
def test_round_trip(variant):
    import torch

    src_slots, dst_slots = [3, 0, 2], [1, 4, 0]
    A = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    B = api.GroundSegmentation().init(120.0, 0.33, n_slots=5, max_points=20000)
    B.debug_set_tuning("import_variant", variant)
    A.reset_maps(odom_z=0.2)
    B.reset_maps(odom_z=-0.4)
    ex.warm_maps(A, src_slots, seed=2200, n_az=130)
    ex.warm_maps(B, [4, 2], seed=2250, frames=1, n_az=100)  # (one destination warm with other contents, two fresh)
    for row_major in (False, True):
        planes = A.export_layers(slots=src_slots, row_major=row_major)
        keep = planes.clone()
        B.import_layers(planes, slots=dst_slots, row_major=row_major)
        again = B.export_layers(slots=dst_slots, row_major=row_major)
        torch.cuda.synchronize()
        assert same_on_device(again, keep), f"row_major={row_major}"
        assert same_on_device(planes, keep), "the import changed its source"
    want = {d: A.map(s).layers() for s, d in zip(src_slots, dst_slots)}
    for d in dst_slots:
        got = B.map(d).layers()
        for name in LAYERS:
            assert same_bits(got[name], want[d][name]), (d, name)
    with pytest.raises(ValueError):
        B.import_layers(planes, ["groundpatch", "ground"], slots=dst_slots)
    with pytest.raises(ValueError):
        B.import_layers(planes[:, :3], slots=dst_slots)
    A.close()
    B.close()


# ---------------------------------------------------------------- 3. continue after a restore

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("eager", [False, True])
def test_continue_after_restore(eager, variant):
    import torch

    slots, other = [2, 0, 3], [4, 1, 0]
    A = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    B = api.GroundSegmentation().init(120.0, 0.33, n_slots=5, max_points=20000)
    B.debug_set_tuning("import_variant", variant)
    for seg in (A, B):
        if eager:
            seg.set_flags(eager_layers=True)
        seg.reset_maps(odom_z=0.0)
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    base = [synth.hdl64_cloud(seed=2300 + k, n_az=140 + 9 * k) for k in range(len(slots))]
    run_frames(A, slots, base, [0, 1], refs=refs)
    state = A.snapshot_maps(slots=slots)
    assert tuple(state["planes"].shape) == (3, 11, A.cols, A.rows) and state["positions"].shape == (3, 2) and state["positions"].dtype == np.float64
    outs_a, wants = run_frames(A, slots, base, [2, 3], refs=refs)
    B.restore_maps(state, slots=other)
    for k, s in enumerate(other):
        assert B.map(s).getPosition() == tuple(state["positions"][k])
    outs_b, _ = run_frames(B, other, base, [2, 3])
    assert_same_outputs(outs_a, outs_b, "restored against original")
    for f, w in enumerate(wants):  # ... and both are what the oracle computes for the four frames
        la, ia, ca, n = outs_b[f]
        for k, nk in enumerate(n):
            assert np.array_equal(la[k, :nk], w[k]["label"]), (f, k)
            assert np.array_equal(ia[k, :nk], w[k]["index"]), (f, k)
            assert ca[k, 0] == len(w[k]["out_points"]), (f, k)
    assert same_on_device(A.export_layers(slots=slots), B.export_layers(slots=other))
    assert_layers_equal_oracle(B, other, refs, "restored")
    assert_layers_equal_oracle(A, slots, refs, "original")
    small = api.GroundSegmentation().init(26.0, 0.33, n_slots=3, max_points=20000)
    with pytest.raises(ValueError):
        small.restore_maps(state)
    small.close()
    A.close()
    B.close()


# ---------------------------------------------------------------- 4. fresh maps

@pytest.mark.parametrize("variant", VARIANTS)
def test_fresh_maps(variant):
    import torch

    B = 100
    clouds = [synth.hdl64_cloud(seed=1500 + k, n_az=96 + (k % 5) * 3) for k in range(B)]
    stride = stride_of(clouds)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    seg.debug_set_tuning("import_variant", variant)
    z = [0.25 if s < 50 else -1.5 for s in range(B)]
    seg.reset_maps(0, 50, odom_z=0.25, on_torch_stream=True)
    seg.reset_maps(50, 50, odom_z=-1.5, on_torch_stream=True)
    refs = [oracle.OracleMap(120.0, 0.33, odom_z=z[s]) for s in range(B)]
    assert fresh_count(seg) == B
    groups = [(["ground"], [5, 77, 50]), (["groundpatch"], [49, 6, 98]), (["ground", "groundpatch"], [0, 99, 51]), (["pointsRaw"], [7, 60, 8])]
    C_ = seg.rows * seg.cols
    pool = random_pool(3 * 2 * C_, seed=44, finite=True)
    for g, (names, slots) in enumerate(groups):
        src = torch.from_numpy(np.roll(pool, 1000 * g)[: 3 * len(names) * C_].copy()).cuda().view(3, len(names), seg.cols, seg.rows)
        seg.import_layers(src, names, slots=slots, row_major=bool(g % 2))
        host = src.cpu().numpy()
        for i, s in enumerate(slots):
            for k, name in enumerate(names):
                refs[s].set_layer(name, host[i, k] if g % 2 else host[i, k].T)
    assert fresh_count(seg) == B - 9
    twelve = [s for _, sl in groups for s in sl]
    planes = seg.export_layers(slots=twelve)
    torch.cuda.synchronize()
    assert fresh_count(seg) == B - 9
    ex.assert_export_equals(planes.cpu().numpy(), seg, twelve, list(LAYERS), lambda s: {k: refs[s].layer(k) for k in LAYERS}, "the twelve")
    # every map -- 91 fresh ones, nine the imports made real, three with an imported pointsRaw -- through one large batch
    origins = np.array([[0.05 * (b % 7), -0.03 * (b % 5), 0.01 * (b % 3)] for b in range(B)], dtype=np.float32)
    base_z = np.array([-1.73 + 0.003 * (b % 9) for b in range(B)])
    out = seg.filter_batch(batch_points(clouds, stride), [len(c) for c in clouds], origins, base_z)
    assert fresh_count(seg) == 0
    planes = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    labels = out.labels.cpu().numpy()
    for s in range(B):
        r = refs[s].filter_cloud(clouds[s], tuple(origins[s]), float(base_z[s]))
        assert np.array_equal(labels[s, : len(clouds[s])], r["label"]), s
    ex.assert_export_equals(planes.cpu().numpy(), seg, list(range(B)), ["ground", "groundpatch"],
                            lambda s: {k: refs[s].layer(k) for k in ("ground", "groundpatch")}, "after the batch")
    seg.close()


# ---------------------------------------------------------------- 5. the lazily kept layers

@pytest.mark.parametrize("variant", VARIANTS)
def test_lazy_layers(variant):
    import torch

    slots = [3, 1, 0]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.debug_set_tuning("import_variant", variant)
    seg.reset_maps(odom_z=0.0)
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    base = [synth.hdl64_cloud(seed=2500 + k, n_az=150) for k in range(len(slots))]
    run_frames(seg, slots, base, [0, 1], refs=refs)  # (the default of filter_batch: the three layers are left out)
    C_ = seg.rows * seg.cols
    one = torch.from_numpy(random_pool(3 * C_, seed=51)).cuda().view(3, 1, seg.cols, seg.rows)
    seg.import_layers(one, ["planeDist"], slots=slots)
    for i, (s, r) in enumerate(zip(slots, refs)):
        r.set_layer("planeDist", one[i, 0].cpu().numpy().T)
    assert_layers_equal_oracle(seg, slots, refs, "planeDist imported, the other two from the last cloud")
    run_frames(seg, slots, base, [2], refs=refs)  # (pending again)
    three = torch.from_numpy(random_pool(3 * 3 * C_, seed=52)).cuda().view(3, 3, seg.cols, seg.rows)
    seg.import_layers(three, LAZY, slots=slots)
    host = three.cpu().numpy()
    for i, r in enumerate(refs):
        for k, name in enumerate(LAZY):
            r.set_layer(name, host[i, k].T)
    assert_layers_equal_oracle(seg, slots, refs, "all three imported")
    run_frames(seg, slots, base, [3], refs=refs)
    assert_layers_equal_oracle(seg, slots, refs, "a batch after the imports")
    seg.close()


# ---------------------------------------------------------------- 6. the sparse per-call layers

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("length,res,size", [(120.0, 0.33, 364), (26.0, 0.33, 79)])
def test_sparse_layers(length, res, size, variant):
    import torch

    seg = api.GroundSegmentation().init(length, res, n_slots=2, max_points=20000)
    assert seg.rows == size
    seg.debug_set_tuning("import_variant", variant)
    seg.reset_maps(odom_z=0.0)
    full = synth.hdl64_cloud(seed=2600, n_az=60)
    near = np.hypot(full["x"], full["y"]) < 9.0  # (a small part of either grid)
    cloud = np.frombuffer(full.view(np.uint8).reshape(-1, 32)[near].tobytes(), dtype=np.uint8).copy().view(synth.POINT_DTYPE)
    assert len(cloud) > 500
    ref = oracle.OracleMap(length, res)
    seg.filter_batch(batch_points([cloud], stride_of([cloud])), [len(cloud)], np.zeros((1, 3), np.float32), np.full(1, -1.73), first_slot=1)
    ref.filter_cloud(cloud, (0.0, 0.0, 0.0), -1.73)
    untouched = ref.layer("pointsRaw") == 0
    assert untouched.mean() > 0.5
    src = torch.from_numpy(random_pool(size * size, seed=61)).cuda().view(1, 1, seg.cols, seg.rows)
    seg.import_layers(src, ["m2"], first_slot=1, n=1)
    ref.set_layer("m2", src[0, 0].cpu().numpy().T)
    got = seg.map(1).layers()
    for name in LAYERS:
        assert same_bits(got[name], ref.layer(name)), name
    assert np.all(bits(got["minGroundHeight"][untouched]) == bits(FLT_MAX)) and np.all(bits(got["maxGroundHeight"][untouched]) == bits(FLT_MIN))
    seg.map(1).detect_ground_patches(-1)
    ref.stage_detect()
    assert_layers_equal_oracle(seg, [1], [ref], "detect_ground_patches on the imported layers")
    seg.close()


# ---------------------------------------------------------------- 7. ordering

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("halves", [False, True])
def test_import_between_two_batches_on_another_stream(halves, variant):
    import torch

    n_slots, slots = 16, [2, 9, 5, 12, 7, 8, 15, 0]  # both halves (boundary 8)
    imported = [9, 0, 7, 12]
    names = ["points", "ground", "groundpatch", "planeDist"]
    K = len(slots)
    base = [synth.hdl64_cloud(seed=1700 + k, n_az=150) for k in range(K)]
    stride = stride_of(base)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride) for _ in range(2)]
    segs[0].debug_set_tuning("import_variant", variant)
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
    C_ = segs[0].rows * segs[0].cols
    # (finite terrain: the two contexts sweep it with different kernels under halves, and a NaN's payload after arithmetic is not part of any contract)
    src = torch.from_numpy(np.abs(random_pool(len(imported) * len(names) * C_, seed=71, finite=True))).cuda().view(len(imported), len(names), segs[0].cols, segs[0].rows)
    torch.cuda.synchronize()  # (the uploads ran on torch's default stream)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        segs[0].filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
    segs[0].import_layers(src, names, slots=imported, stream=b.cuda_stream)  # no synchronisation in between: the library orders it
    with torch.cuda.stream(a):
        segs[0].move_maps(odoms, [ex.POSE] * K, slots=slots, on_torch_stream=True)
        out0 = segs[0].filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    # the same sequence on the other context, one step at a time
    segs[1].filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    segs[1].import_layers(src, names, slots=imported)
    torch.cuda.synchronize()
    segs[1].move_maps(odoms, [ex.POSE] * K, slots=slots, on_torch_stream=True)
    out1 = segs[1].filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
    torch.cuda.synchronize()
    assert torch.equal(out0.counts, out1.counts)
    for k in range(K):
        assert torch.equal(out0.labels[k, : n_pts[1][k]], out1.labels[k, : n_pts[1][k]]), k
    for s in range(n_slots):
        got, want = segs[0].map(s).layers(), segs[1].map(s).layers()
        for name in LAYERS:
            assert same_bits(got[name], want[name]), (s, name)
    for seg in segs:
        seg.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_torch_op_right_behind_the_import(variant):
    import torch

    slots, names = [1, 3, 0], ["ground", "groundpatch", "variance"]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=5, max_points=20000)
    seg.debug_set_tuning("import_variant", variant)
    seg.reset_maps(odom_z=0.2)
    ex.warm_maps(seg, slots, seed=1800, frames=1, n_az=100)
    host = np.abs(random_pool(3 * 3 * seg.rows * seg.cols, seed=81)).reshape(3, 3, seg.cols, seg.rows)
    host[~np.isfinite(host)] = np.float32(0.5)  # (2 x inf = inf and 2 x NaN keeps its payload, but keep the doubling exact and plain)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        planes = torch.from_numpy(host).cuda()
        seg.import_layers(planes, names, slots=slots)
        planes2 = planes * 2.0  # (same stream, no synchronise in between)
        planes.zero_()          # ... and the source rewritten right behind the call that reads it
        seg.import_layers(planes2, names, slots=[2, 4, 0])
    stream.synchronize()
    for i, s in enumerate([1, 3]):
        got = seg.map(s).layers(names)
        for k, name in enumerate(names):
            assert same_bits(got[name], host[i, k].T), (s, name)
    for i, s in enumerate([2, 4, 0]):
        got = seg.map(s).layers(names)
        for k, name in enumerate(names):
            assert same_bits(got[name], (host[i, k] * np.float32(2.0)).T), (s, name)
    seg.close()


# ---------------------------------------------------------------- 8. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    seg.reset_maps(odom_z=0.4)
    ex.warm_maps(seg, [4, 1], seed=1900, frames=1, n_az=100)
    C_ = seg.rows * seg.cols
    names = ["ground", "groundpatch", "planeDist"]
    mask = mask_of(names)
    before = seg.export_layers()
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    src = torch.from_numpy(random_pool(2 * 3 * C_, seed=91)).cuda()
    p = src.data_ptr()
    INVALID, CAPACITY = -1, -5
    col = _lib.GG_PLANES_COLMAJOR
    assert seg._L.gg_import_layers(None, 2, None, 0, mask, col, C.c_void_p(p), C_, None) == INVALID
    assert seg._L.gg_import_layers(None, 0, None, 0, mask, col, C.c_void_p(p), C_, None) == INVALID
    assert raw_import(seg, -1, None, 0, mask, col, p, C_) == INVALID
    assert raw_import(seg, 2, [1, 1], 0, mask, col, p, C_) == INVALID
    assert raw_import(seg, 2, None, 0, mask | (1 << _lib.GG_NUM_LAYERS), col, p, C_) == INVALID
    assert raw_import(seg, 2, None, 0, 0, col, p, C_) == INVALID
    assert raw_import(seg, 2, None, 0, mask, 2, p, C_) == INVALID
    assert raw_import(seg, 2, None, 0, mask, -1, p, C_) == INVALID
    assert raw_import(seg, 2, None, 0, mask, col, None, C_) == INVALID
    assert raw_import(seg, 2, None, 0, mask, col, p, C_ - 1) == INVALID
    assert raw_import(seg, 2, [1, 6], 0, mask, col, p, C_) == CAPACITY
    assert raw_import(seg, 2, [-1, 2], 0, mask, col, p, C_) == CAPACITY
    assert raw_import(seg, 2, None, 5, mask, col, p, C_) == CAPACITY
    assert raw_import(seg, 2, None, -1, mask, col, p, C_) == CAPACITY
    assert raw_import(seg, 0, None, 0, 0, 7, None, 0) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers()
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    assert same_on_device(before, after)
    seg.close()
