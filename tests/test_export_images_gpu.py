"""gg_export_images (the 8-bit layer images and the 32FC3 terrain images of many maps in device memory, one call) on the device: byte
for byte what gg_get_layer_image_u8 returns and bit for bit what gg_get_terrain_image returns per map, taken from a twin context that
went through the same calls -- fresh maps, lazily kept layers, planes with NaN / inf / -0.0 / denormals, a constant layer, a layer
without a finite cell, odd destination addresses and strides, caller streams, GG_FLAG_CONCURRENT_HALVES -- tied to the CPU oracle as
well, and errors that change nothing.  Every comparison is exact; there is no tolerance."""
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
from tests.seq_model import image_u8_reference, terrain_reference  # noqa: E402
from tests.test_export_layers_gpu import POSE, SENTINEL, batch_points, bits, fresh_count, mask_of, same_bits, sentinel_tensor, stride_of, warm_maps  # noqa: E402

pytestmark = pytest.mark.gpu

LAZY = ["maxGroundHeight", "groundCandidates", "planeDist"]
U8_MASKS = [["ground"], ["groundpatch"], ["planeDist"], LAZY, ["points", "pointsRaw", "variance"], list(LAYERS)]
BYTE = 0xA5  # (the sentinel of the byte destinations)
GAP = 37
INVALID, CAPACITY = -1, -5


def raw_images(seg, n, slots, first_slot, mask, images=0, image_stride=0, bounds=0, terrain=0, terrain_stride=0, layout=0, stream=None, own=False):
    """gg_export_images as the C ABI has it (device addresses as integers, 0 = null); returns the status"""
    import torch

    x = _lib.GGImageExport()
    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    x.n, x.first_slot, x.slots, x.layer_mask = n, first_slot, sl, mask
    x.d_images, x.image_stride, x.d_bounds = images or None, image_stride, bounds or None
    x.d_terrain, x.terrain_stride, x.terrain_layout = terrain or None, terrain_stride, layout
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_export_images(seg._ctx, C.byref(x), None if own else C.c_void_p(s if s else _lib.GG_STREAM_DEFAULT))


def byte_tensor(count):
    import torch

    return torch.full((count,), BYTE, dtype=torch.uint8, device="cuda")


def special_plane(rows, cols, seed):
    """a plane of ordinary values with a NaN that carries a payload, both infinities, -0.0 and denormals -- corners and interior"""
    g = np.random.default_rng(seed).normal(size=(rows, cols)).astype(np.float32)
    u = g.view(np.uint32)
    u[0, 0] = 0x7FC12345
    u[rows // 2, cols // 3] = 0xFFC00001
    g[0, cols - 1] = np.inf
    g[rows - 1, 0] = -np.inf
    u[rows - 1, cols - 1] = 0x80000000  # -0.0
    u[1, 1] = 0x00000311                # a denormal
    u[rows // 3, cols // 2] = 0x80000007
    g[2, 5] = np.float32(3.0e38)
    return g


def build_scene(seg, n_slots, seed):
    """Slot 0 stays fresh; the others are warmed (scrolled, sparse per-call layers, lazily kept layers pending).  With six slots, 3 is
    re-initialised after its clouds, 4 holds set planes with special values, 5 a constant layer and a layer without a finite cell."""
    rows, cols = seg.rows, seg.cols
    seg.reset_maps(odom_z=0.3)
    warm_maps(seg, list(range(1, n_slots)), seed=seed)
    if n_slots >= 6:
        seg.map(4).set("ground", special_plane(rows, cols, seed + 1))
        seg.map(4).set("m2", special_plane(rows, cols, seed + 2))
        seg.map(5).set("variance", np.full((rows, cols), 2.5, dtype=np.float32))
        none = np.full((rows, cols), np.nan, dtype=np.float32)
        none[::7, ::5] = np.inf
        none[3::11, 1::4] = -np.inf
        seg.map(5).set("meanVariance", none)
        seg.reset_maps(3, 1, odom_z=-0.7)
    else:
        seg.map(1).set("ground", special_plane(rows, cols, seed + 1))
    seg.reset_maps(0, 1, odom_z=0.3)  # (the single-map setters above filled it)
    import torch

    torch.cuda.synchronize()  # (not seg.synchronize(): like every call on the context's own stream it fills the fresh maps)
    return 2 if n_slots >= 6 else 1  # fresh maps


def twins(length, res, n_slots, seed, max_points=20000):
    segs = [api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=max_points) for _ in range(2)]
    n_fresh = [build_scene(seg, n_slots, seed) for seg in segs]
    assert fresh_count(segs[0]) == n_fresh[0]
    return segs


def selections(n_slots, seed=9):
    subset = [int(s) for s in np.random.default_rng(seed).permutation(n_slots)[: max(2, n_slots - 1)]]
    if 0 not in subset:
        subset[-1] = 0  # (the fresh map is in the permuted list)
    return [(subset, 0, len(subset)), (None, 1, n_slots - 1)]


def getter_images(seg, names=LAYERS):
    """{(slot, layer): (image, lower, upper)} from the single getter"""
    return {(s, k): seg.map(s).image_u8(k) for s in range(seg.n_slots) for k in names}


def check_images(flat, offset, stride, sl, names, want, C_, tag):
    """flat: the downloaded byte destination; image k of map i starts at offset + (i * K + k) * stride"""
    K = len(names)
    assert np.all(flat[:offset] == BYTE), f"{tag}: bytes in front of the first image were written"
    for i, s in enumerate(sl):
        for k, name in enumerate(names):
            at = offset + (i * K + k) * stride
            got, ref = flat[at: at + C_], want[(s, name)][0].reshape(-1)
            assert np.array_equal(got, ref), f"{tag}: map {i} (slot {s}) layer {name}: {int((got != ref).sum())} bytes differ"
            assert np.all(flat[at + C_: at + stride] == BYTE), f"{tag}: the gap behind image {k} of map {i} was written"
    assert np.all(flat[offset + len(sl) * K * stride:] == BYTE), f"{tag}: bytes behind the last image were written"


def check_bounds(b, sl, names, want, tag):
    for i, s in enumerate(sl):
        for k, name in enumerate(names):
            lo, hi = np.float32(want[(s, name)][1]), np.float32(want[(s, name)][2])
            assert b[i, k, 0] == lo and b[i, k, 1] == hi, f"{tag}: map {i} (slot {s}) layer {name}: bounds {b[i, k]} against ({lo}, {hi})"


# ---------------------------------------------------------------- 1. parity with gg_get_layer_image_u8

@pytest.mark.parametrize("size,n_slots,variant", [(79, 6, 0), (79, 6, 1), (364, 6, 0), (364, 6, 1), (1000, 2, 0)])
def test_u8_parity_with_the_getter(size, n_slots, variant):
    import torch

    length, res = {79: (26.0, 0.33), 364: (120.0, 0.33), 1000: (200.0, 0.2)}[size]
    A, B = twins(length, res, n_slots, seed=2100)
    assert A.rows == A.cols == size
    A.debug_set_tuning("images_variant", variant)
    C_ = size * size
    stride = C_ + GAP
    fresh_before = fresh_count(A)
    got = []
    for names in U8_MASKS:
        for slots, first, n in selections(n_slots):
            K = len(names)
            dst = byte_tensor(n * K * stride + 9)
            assert dst.data_ptr() % 2 == 0
            bounds = sentinel_tensor(n * K * 2) if slots is not None else None  # (the range calls keep the bounds in the call's scratch)
            rc = raw_images(A, n, slots, first, mask_of(names), dst.data_ptr() + 1, stride, bounds.data_ptr() if bounds is not None else 0)
            assert rc == 0, A._L.gg_last_error(A._ctx)
            assert fresh_count(A) == fresh_before
            got.append((names, slots if slots is not None else list(range(first, first + n)), dst, bounds))
    torch.cuda.synchronize()
    assert fresh_count(A) == fresh_before
    host = [(names, sl, dst.cpu().numpy(), None if b is None else b.cpu().numpy().reshape(len(sl), len(names), 2)) for names, sl, dst, b in got]
    want = getter_images(B)
    assert want[(0, "ground")][1] == want[(0, "ground")][2] == np.float32(0.3)  # (the fresh map: a constant plane)
    if n_slots >= 6:
        assert want[(5, "variance")][1] == want[(5, "variance")][2] == 2.5
        assert want[(5, "meanVariance")][1] == np.inf and want[(5, "meanVariance")][2] == -np.inf
    for names, sl, flat, b in host:
        tag = f"{size} variant {variant} {'+'.join(names) if len(names) < 11 else 'all'}"
        check_images(flat, 1, stride, sl, names, want, C_, tag)
        if b is not None:
            check_bounds(b, sl, names, want, tag)
    for seg in (A, B):
        seg.close()


# ---------------------------------------------------------------- 2. terrain

@pytest.mark.parametrize("size,variant", [(79, 0), (79, 1), (364, 0), (364, 1)])
def test_terrain_parity_with_the_getter(size, variant):
    import torch

    n_slots = 6
    length, res = {79: (26.0, 0.33), 364: (120.0, 0.33)}[size]
    A, B = twins(length, res, n_slots, seed=2200)
    A.debug_set_tuning("images_variant", variant)
    C_ = size * size
    tstride, stride = 3 * C_ + GAP, C_ + GAP
    with_names = ["ground", "pointsRaw"]
    fresh_before = fresh_count(A)
    got = []
    for layout in (_lib.GG_TERRAIN_HWC, _lib.GG_TERRAIN_CHW):
        for slots, first, n in selections(n_slots):
            for names in ([], with_names):  # terrain alone (mask 0), and with u8 images in the same call
                ter = sentinel_tensor(n * tstride)
                img = byte_tensor(n * len(names) * stride + 9) if names else None
                rc = raw_images(A, n, slots, first, mask_of(names), img.data_ptr() + 1 if names else 0, stride, 0, ter.data_ptr(), tstride, layout)
                assert rc == 0, A._L.gg_last_error(A._ctx)
                assert fresh_count(A) == fresh_before
                got.append((layout, names, slots if slots is not None else list(range(first, first + n)), ter, img))
    torch.cuda.synchronize()
    host = [(layout, names, sl, ter.cpu().numpy(), None if img is None else img.cpu().numpy()) for layout, names, sl, ter, img in got]
    want = {s: B.map(s).terrain_image() for s in range(n_slots)}
    want_u8 = getter_images(B, with_names)
    for layout, names, sl, flat, img in host:
        tag = f"{size} variant {variant} {'CHW' if layout else 'HWC'} {'with images' if names else 'alone'}"
        for i, s in enumerate(sl):
            t = flat[i * tstride: i * tstride + 3 * C_]
            ref = want[s] if layout == _lib.GG_TERRAIN_HWC else want[s].transpose(2, 0, 1)
            assert same_bits(t, ref.reshape(-1)), f"{tag}: map {i} (slot {s}): {int((bits(t) != bits(ref.reshape(-1))).sum())} floats differ"
            assert np.all(flat[i * tstride + 3 * C_: (i + 1) * tstride].view(np.uint32) == SENTINEL), f"{tag}: the gap behind map {i} was written"
            if s == 0:  # the fresh map: channel 0 is odom_z
                ch0 = t.reshape(size, size, 3)[:, :, 0] if layout == _lib.GG_TERRAIN_HWC else t[:C_]
                assert np.all(bits(ch0) == bits(np.float32(0.3)))
        if names:
            check_images(img, 1, stride, sl, names, want_u8, C_, tag)
    for seg in (A, B):
        seg.close()


# ---------------------------------------------------------------- 3. against the reference semantics

@pytest.mark.parametrize("variant", [0, 1])
def test_against_the_oracle(variant):
    import torch

    slots = [3, 0, 5, 2]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    seg.debug_set_tuning("images_variant", variant)
    for s in slots:
        seg.map(s).reset()
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    warm_maps(seg, slots, seed=2300, frames=3, refs=refs)
    res = seg.export_images(terrain=True, slots=slots, on_torch_stream=True)
    chw = seg.export_images([], terrain=True, chw=True, slots=slots, on_torch_stream=True)
    torch.cuda.synchronize()
    images, bounds, terrain, planes = res.images.cpu().numpy(), res.bounds.cpu().numpy(), res.terrain.cpu().numpy(), chw.terrain.cpu().numpy()
    for i, s in enumerate(slots):
        for k, name in enumerate(LAYERS):
            img, lo, hi = image_u8_reference(refs[i].layer(name))
            assert np.array_equal(images[i, k], img), f"slot {s} layer {name}: {int((images[i, k] != img).sum())} bytes differ"
            assert bounds[i, k, 0] == lo and bounds[i, k, 1] == hi, (s, name, bounds[i, k], lo, hi)
        ground, raw = refs[i].layer("ground"), refs[i].layer("pointsRaw")
        t = terrain_reference(ground, raw)
        assert "visited" in t  # (pointsRaw holds counts: the 3 x 3 sum does not depend on the order)
        assert np.array_equal(terrain[i, :, :, 0], ground, equal_nan=True) and np.array_equal(terrain[i, :, :, 2], raw, equal_nan=True), s
        assert np.array_equal(terrain[i, 1:-1, 1:-1, 1], t["visited"]), s
        assert not terrain[i, 0, :, 1].any() and not terrain[i, -1, :, 1].any() and not terrain[i, :, 0, 1].any() and not terrain[i, :, -1, 1].any()
        assert same_bits(planes[i], terrain[i].transpose(2, 0, 1)), s
    seg.close()


# ---------------------------------------------------------------- 4. the state afterwards

def test_state_after_the_exports():
    import torch

    n_slots = 6
    A, B = twins(120.0, 0.33, n_slots, seed=2400)
    everything = list(range(n_slots))
    res = A.export_images(terrain=True, slots=everything, on_torch_stream=True)  # (the lazily kept layers: computed by the call in A ...)
    torch.cuda.synchronize()
    want = getter_images(B)                                                      # (... and by the getters in B)
    images, bounds = res.images.cpu().numpy(), res.bounds.cpu().numpy()
    for s in everything:
        for k, name in enumerate(LAYERS):
            assert np.array_equal(images[s, k], want[(s, name)][0]), (s, name)
        assert same_bits(res.terrain[s].cpu().numpy(), B.map(s).terrain_image()), s
    check_bounds(bounds, everything, list(LAYERS), want, "all slots")
    clouds = [synth.hdl64_cloud(seed=2450 + k, n_az=170 + 7 * k) for k in range(n_slots)]
    stride = stride_of(clouds)
    pts = batch_points(clouds, stride)
    n_pts, origins, base_z = [len(c) for c in clouds], np.zeros((n_slots, 3), np.float32), np.full(n_slots, -1.73)
    outs = [seg.filter_batch(pts, n_pts, origins, base_z, slots=everything) for seg in (A, B)]
    planes = [seg.export_layers() for seg in (A, B)]
    torch.cuda.synchronize()
    for field in ("labels", "out_index", "counts"):
        a, b = getattr(outs[0], field).cpu().numpy(), getattr(outs[1], field).cpu().numpy()
        if field == "counts":
            assert np.array_equal(a, b)
        else:
            for k in range(n_slots):
                assert np.array_equal(a[k, : n_pts[k]], b[k, : n_pts[k]]), (field, k)
    assert same_bits(planes[0].cpu().numpy(), planes[1].cpu().numpy())
    for seg in (A, B):
        seg.close()


# ---------------------------------------------------------------- 5. a caller's stream, no host synchronisation

@pytest.mark.parametrize("halves", [False, True])
def test_on_a_caller_stream_past_the_ring(halves):
    import torch

    n_slots, slots = 16, [2, 9, 5, 12, 7, 8, 15, 0]  # both halves (boundary 8)
    listed = slots + [3]                              # (3 is never in a batch: fresh at every export)
    K = len(slots)
    names = ["ground", "groundpatch", "planeDist", "pointsRaw"]
    base = [synth.hdl64_cloud(seed=2500 + k, n_az=150) for k in range(K)]
    stride = stride_of(base)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride) for _ in range(2)]
    if halves:
        segs[0].set_flags(concurrent_halves=True)
        segs[0].debug_set_tuning("halves_min_clouds", 2)
    pts = [batch_points(base, stride), batch_points(base[::-1], stride)]
    n_pts = [[len(c) for c in base], [len(c) for c in base[::-1]]]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    rounds = 3  # two exports each: past the four entries of the export ring
    odoms = [np.array([(1.1 * (1 + (k + r) % 3), -0.8 * ((k + r) % 2)) for k in range(K)]) for r in range(rounds)]
    torch.cuda.synchronize()  # (the uploads ran on torch's default stream)

    def sequence(seg, read):
        """the loop on `seg`; read(seg) is called at the two points of every round"""
        taken = []
        for r in range(rounds):
            seg.reset_maps(odom_z=0.1 * r, on_torch_stream=True)
            seg.filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots)
            taken.append(read(seg))
            seg.move_maps(odoms[r], [POSE] * K, slots=slots, on_torch_stream=True)
            seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
            taken.append(read(seg))
        return taken

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = sequence(segs[0], lambda seg: seg.export_images(names, terrain=True, slots=listed, on_torch_stream=True))  # no synchronisation anywhere
    torch.cuda.synchronize()

    def getters(seg):
        torch.cuda.synchronize()
        return {s: ({k: seg.map(s).image_u8(k) for k in names}, seg.map(s).terrain_image()) for s in listed}

    want = sequence(segs[1], getters)
    for step, (res, ref) in enumerate(zip(got, want)):
        images, bounds, terrain = res.images.cpu().numpy(), res.bounds.cpu().numpy(), res.terrain.cpu().numpy()
        for i, s in enumerate(listed):
            for k, name in enumerate(names):
                img, lo, hi = ref[s][0][name]
                assert np.array_equal(images[i, k], img), f"export {step}: slot {s} layer {name}: {int((images[i, k] != img).sum())} bytes differ"
                assert bounds[i, k, 0] == np.float32(lo) and bounds[i, k, 1] == np.float32(hi), (step, s, name)
            assert same_bits(terrain[i], ref[s][1]), f"export {step}: slot {s}: terrain"
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 6. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000)
    seg.reset_maps(odom_z=0.4)
    warm_maps(seg, [4, 1], seed=2600, frames=1)
    C_ = seg.rows * seg.cols
    names = ["ground", "groundpatch", "planeDist"]
    mask = mask_of(names)
    before = seg.export_layers(names)
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    img, bnd, ter = byte_tensor(2 * 3 * C_), sentinel_tensor(2 * 3 * 2), sentinel_tensor(2 * 3 * C_)
    pi, pb, pt = img.data_ptr(), bnd.data_ptr(), ter.data_ptr()
    hwc = _lib.GG_TERRAIN_HWC

    def call(n=2, slots=None, first=0, mask=mask, images=pi, image_stride=C_, bounds=pb, terrain=pt, terrain_stride=3 * C_, layout=hwc):
        return raw_images(seg, n, slots, first, mask, images, image_stride, bounds, terrain, terrain_stride, layout)

    x = _lib.GGImageExport()
    x.n, x.layer_mask, x.d_images, x.image_stride = 2, mask, pi, C_
    assert seg._L.gg_export_images(None, C.byref(x), None) == INVALID
    assert seg._L.gg_export_images(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(slots=[1, 1]) == INVALID
    assert call(mask=mask | (1 << _lib.GG_NUM_LAYERS)) == INVALID
    assert call(images=0) == INVALID                      # a mask and no destination
    assert call(mask=0, terrain=0) == INVALID             # nothing asked for
    assert call(image_stride=C_ - 1) == INVALID
    assert call(terrain_stride=3 * C_ - 1) == INVALID
    assert call(mask=0, images=0, terrain_stride=3 * C_ - 1) == INVALID
    assert call(layout=2) == INVALID
    assert call(layout=-1) == INVALID
    assert call(slots=[1, 6]) == CAPACITY
    assert call(slots=[-1, 2]) == CAPACITY
    assert call(first=5) == CAPACITY
    assert call(first=-1) == CAPACITY
    assert call(n=0, mask=0, images=0, bounds=0, terrain=0, image_stride=0, terrain_stride=0, layout=7) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert np.all(img.cpu().numpy() == BYTE)
    assert np.all(bnd.cpu().numpy().view(np.uint32) == SENTINEL) and np.all(ter.cpu().numpy().view(np.uint32) == SENTINEL)
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(names)
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    assert call() == 0, seg._L.gg_last_error(seg._ctx)  # ... and the same arguments without a mistake are accepted
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    seg.close()


# ---------------------------------------------------------------- 7. the Python entry point

def test_python_entry_point_shapes_and_out():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.reset_maps(odom_z=0.1)
    warm_maps(seg, [2, 0, 3], seed=2700, frames=1)
    rows, cols = seg.rows, seg.cols
    a = seg.export_images(on_torch_stream=True)
    assert a.images.shape == (4, 11, rows, cols) and a.images.dtype == torch.uint8 and a.images.is_cuda
    assert a.bounds.shape == (4, 11, 2) and a.bounds.dtype == torch.float32 and a.terrain is None
    b = seg.export_images(["ground", "pointsRaw"], terrain=True, slots=[3, 0], on_torch_stream=True)
    assert b.images.shape == (2, 2, rows, cols) and b.bounds.shape == (2, 2, 2)
    assert b.terrain.shape == (2, rows, cols, 3) and b.terrain.dtype == torch.float32
    c = seg.export_images([], terrain=True, chw=True, first_slot=2, n=2, on_torch_stream=True)
    assert c.images is None and c.bounds is None and c.terrain.shape == (2, 3, rows, cols)
    again = seg.export_images(["ground", "pointsRaw"], terrain=True, slots=[0, 3], out=b, on_torch_stream=True)  # (its tensors are reused)
    assert again is b
    own = seg.export_images(["groundpatch"], first_slot=1, n=1)  # the context's own stream
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        seg.export_images(["groundpatch", "ground"])
    with pytest.raises(ValueError):
        seg.export_images([])
    with pytest.raises(ValueError):
        seg.export_images(["ground"], out=b)
    torch.cuda.synchronize()
    want = getter_images(seg)
    ter = {s: seg.map(s).terrain_image() for s in range(4)}
    images, bounds = a.images.cpu().numpy(), a.bounds.cpu().numpy()
    for s in range(4):
        for k, name in enumerate(LAYERS):
            assert np.array_equal(images[s, k], want[(s, name)][0]), (s, name)
    check_bounds(bounds, [0, 1, 2, 3], list(LAYERS), want, "all")
    for i, s in enumerate([0, 3]):
        for k, name in enumerate(["ground", "pointsRaw"]):
            assert np.array_equal(b.images[i, k].cpu().numpy(), want[(s, name)][0]), (s, name)
        assert same_bits(b.terrain[i].cpu().numpy(), ter[s]), s
    for i, s in enumerate([2, 3]):
        assert same_bits(c.terrain[i].cpu().numpy(), ter[s].transpose(2, 0, 1)), s
    assert np.array_equal(own.images[0, 0].cpu().numpy(), want[(1, "groundpatch")][0])
    seg.close()
