"""gg_create's two sensor constants (gg_geometry.vertical_point_ang_dist / min_dist_squared) away from their defaults, on the device, bit for
bit against the oracle created with the same constants (tests/geom_sets.py: the constant sets A .. F and why each is where it is;
tests/test_geometry_constants_cpu.py: these scenes can see the decay threshold one off, the ignore compare one float off and a table
built with the wrong vertical_point_ang_dist).  Every launch shape that restates `dx^2 + dy^2 >= r2min` with an index expression of its
own is run at every set: the pair sweep (one cloud), k_sweep in parts (24 clouds), k_sweep<FRESH> (> 256 fresh maps, plain and as two
concurrent halves), the throughput pair sweep (forced); at least four frames per map on clouds that shrink, so that cells lose their
observations and the decay acts.  All 11 layers, labels, emission index, counts and the returned cloud's bytes.  Nothing here reads the
reference tree."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from groundgrid_amd import _lib, api  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import geom_sets as gs  # noqa: E402
from tests.test_gpu_parity import _batch_inputs, _check_batch_against_oracle, assert_same_state, nan_equal, run_pair  # noqa: E402
from tests.test_gpu_stages_wire import synthetic_layers  # noqa: E402

ALL = sorted(gs.SETS)


def shrink(frame, n):
    return gs.frame_points(n, frame)


def make_seg(name, n_slots, max_points):
    L, R, vpad, mds = gs.geometry(name)
    return api.GroundSegmentation().init(L, R, n_slots=n_slots, max_points=max_points, vertical_point_ang_dist=vpad, min_dist_squared=mds)


# ---------------------------------------------------------------- one cloud per call: the pair sweep
@pytest.mark.parametrize("name", ALL)
def test_one_cloud_per_call(name):
    L, R, vpad, mds = gs.geometry(name)
    sc = gs.scene(name)
    r = run_pair(sc.cloud, length=L, resolution=R, origin=sc.origin, base_z=sc.base_z, frames=sc.frames, geom=(vpad, mds), n_points=shrink)
    if name == "D":   # every in-map point is ignored: the returned cloud is the ignored block alone
        assert (r["cls"] != oracle.KEPT).all() and (r["cls"] != oracle.OUTLIER).all() and (r["cls"] == oracle.IGNORED).sum() > 1000
        assert len(r["out_points"]) == ((r["cls"] == oracle.IGNORED) & (r["index"] >= 0)).sum() > 0
    else:
        assert (r["cls"] == oracle.KEPT).sum() > 1000
    if name in "ABC":
        assert (r["cls"] == oracle.IGNORED).sum() > 100


# ---------------------------------------------------------------- batches: k_sweep in parts, fresh maps, concurrent halves, throughput pair sweep
def run_batch(name, shape, fmt):
    L, R, vpad, mds = gs.geometry(name)
    B = gs.BATCH_COUNTS[shape]
    clouds = gs.batch_clouds(name, B)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = make_seg(name, B, stride)
    odom_z = 0.0
    if shape in ("fresh", "halves"):
        odom_z = 0.25
        if shape == "halves":
            seg.set_flags(concurrent_halves=True)
        seg.reset_maps(odom_z=odom_z)
    if shape == "throughput":
        seg.debug_set_tuning("sweep_pair", 4)   # as test_throughput_pair_sweep_shapes forces it
    pts = _batch_inputs(fmt, clouds, stride)
    origins = np.array([gs.batch_origin(name)] * B, dtype=np.float32)
    watched = set(range(B)) if B <= 64 else {0, 1, B // 2 - 1, B // 2, B - 1} | set(range(7, B, 32))
    _check_batch_against_oracle(seg, clouds, pts, origins, np.full(B, gs.BATCH_BASE_Z), gs.FRAMES, watched, tag=f"set {name} {shape}",
                                make_ref=lambda: gs.oracle_map(name, odom_z=odom_z), n_points=shrink,
                                after_call=seg.batch_fence if shape == "halves" else None)
    seg.close()


@pytest.mark.parametrize("name", ALL)
def test_batch_swept_in_parts(name):
    run_batch(name, "parts", 32)


@pytest.mark.parametrize("name", ALL)
def test_batch_of_fresh_maps(name):
    run_batch(name, "fresh", 16)


@pytest.mark.parametrize("name", ALL)
def test_batch_of_fresh_maps_in_concurrent_halves(name):
    run_batch(name, "halves", 16)


@pytest.mark.parametrize("name", ALL)
def test_throughput_pair_sweep(name):
    run_batch(name, "throughput", 32)


# ---------------------------------------------------------------- the stage members
def pair_with_layers(name, layers):
    seg = make_seg(name, 1, 64)
    ref = gs.oracle_map(name)
    for k, arr in layers.items():
        seg.map(0).set(k, arr)
        ref.set_layer(k, arr)
    return seg, ref


def test_interpolate_cell_on_the_strict_boundary():
    """k7_stage restates :463 in double where the sweeps compare integers.  Set B: cells with dx^2 + dy^2 = 4225 (on the boundary: no decay)
    on all four sides and off the axes, 4226 (just outside: decay), and their neighbours inside."""
    L, R, vpad, mds = gs.geometry("B")
    n = gs.cells(L, R)
    c = n // 2 - 1
    seg, ref = pair_with_layers("B", synthetic_layers(n, seed=11))
    on = [(a, b) for a, b in ((65, 0), (16, 63), (25, 60), (33, 56), (39, 52))]
    cells = []
    for a, b in on:
        for sa in (-1, 1):
            for sb in (-1, 1):
                cells += [(sa * a, sb * b), (sb * b, sa * a)]
    on_cells = sorted(set(cells))
    outside = [(65, 1), (-65, 1), (1, 65), (1, -65), (-65, -1), (64, 12), (17, 63), (-16, 64)]
    inside = [(64, 0), (0, -64), (16, 62), (-25, 59), (64, 11), (45, 46)]
    for dx, dy in outside:
        assert dx * dx + dy * dy > 4225
    for dx, dy in inside:
        assert dx * dx + dy * dy < 4225
    before = {k: ref.layer("groundpatch")[c + k[0], c + k[1]] for k in on_cells + outside + inside}
    for dx, dy in on_cells + outside + inside:
        assert dx * dx + dy * dy == 4225 or (dx, dy) not in on_cells
        seg.map(0).interpolate_cell(c + dx, c + dy)
        ref.interpolate_cell(c + dx, c + dy)
    for name in ("ground", "groundpatch"):
        assert nan_equal(seg.map(0)[name], ref.layer(name)), name
    after = ref.layer("groundpatch")
    assert all(after[c + k[0], c + k[1]] == before[k] for k in on_cells + inside)   # strict >: the boundary itself does not decay
    assert all(after[c + k[0], c + k[1]] != before[k] or before[k] == 0.0 for k in outside)
    assert sum(before[k] != 0.0 for k in outside) >= 4
    seg.close()


@pytest.mark.parametrize("name", ALL)
def test_spiral_and_detect_patches_stages(name):
    n = gs.cells(*gs.geometry(name)[:2])
    seg, ref = pair_with_layers(name, synthetic_layers(n, seed=5 * n))
    for section in (1, 3, 0, 2):
        seg.map(0).detect_ground_patches(section)
        ref.stage_detect_section(section)
    assert_same_state(seg.map(0), ref, f"set {name} detect_ground_patches")
    for base_z in (-1.73, 0.25):
        seg.map(0).spiral_ground_interpolation(base_z)
        ref.stage_spiral(base_z)
        assert_same_state(seg.map(0), ref, f"set {name} spiral {base_z}")
    seg.map(0).detect_ground_patches(-1)
    ref.stage_detect()
    assert_same_state(seg.map(0), ref, f"set {name} detect on the swept map")
    seg.close()


@pytest.mark.parametrize("name", ALL)
def test_insert_cloud_classes_and_cells(name):
    sc = gs.scene(name)
    cloud = sc.cloud
    seg = make_seg(name, 1, len(cloud))
    ref = gs.oracle_map(name)
    seg.map(0).reset()
    for frame in range(2):   # a warm map for the second insert
        seg.filter_cloud(cloud, sc.origin, sc.base_z)
        r = ref.filter_cloud(cloud, sc.origin, sc.base_z)
        cls, cell = seg.point_classes(len(cloud))
        assert np.array_equal(cls, r["cls"]) and np.array_equal(cell, r["cell"]), frame
    half = len(cloud) // 2
    icls, icell = seg.map(0).insert_cloud(cloud, 0, half, sc.origin)
    ocls, ocell = ref.stage_insert(cloud[:half], sc.origin)
    assert np.array_equal(icls, ocls) and np.array_equal(icell, ocell)
    assert np.array_equal(icls == oracle.IGNORED, cls[:half] == oracle.IGNORED)   # the ignore test does not depend on the map's state
    assert_same_state(seg.map(0), ref, f"set {name} insert_cloud")
    seg.close()


@pytest.mark.parametrize("name", ALL)
def test_expected_points_table(name):
    seg = make_seg(name, 1, 16)
    want = gs.oracle_map(name).expected_points()
    assert np.array_equal(seg.expected_points().view(np.uint32), want.view(np.uint32))
    if gs.geometry(name)[2]:
        L, R = gs.geometry(name)[:2]
        assert not np.array_equal(want, oracle.OracleMap(L, R).expected_points())
    seg.close()


@pytest.mark.parametrize("name", ["A", "B", "F"])
def test_two_per_slot_configurations(name):
    """gg_set_slot_configs builds a patch table per configuration from the context's expected-points table: under a non-default
    vertical_point_ang_dist, two slots with configurations of their own and one that follows the context's"""
    def edit1(c):
        # (set F: its table is 1 / 1e-8 over the default sensor's, beyond any count under the context's threshold and under edit2's, so no
        # slot would find a patch and all three would agree; this threshold brings slot 0's table back to what a default sensor has at 0.6)
        c.ground_patch_detection_minimum_point_count_threshold = 0.6 if name != "F" else 0.6 * 1e-8 / gs.DEFAULT_VPAD
        c.patch_size_change_distance = 8.0

    def edit2(c):
        c.ground_patch_detection_minimum_point_count_threshold = 0.05
        c.occupied_cells_decrease_factor = 3.0
        c.max_ring = 40

    clouds = gs.batch_clouds(name, 3, n_az=200)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = make_seg(name, 3, stride)
    cfgs = []
    for e in (edit1, edit2):
        c = api.default_config()
        e(c)
        cfgs.append(c)
    seg.set_slot_configs(cfgs, slots=[0, 2])
    refs = []

    def make_ref():
        m = gs.oracle_map(name)
        k = len(refs)
        if k == 0:
            edit1(m.cfg)
        elif k == 2:
            edit2(m.cfg)
        refs.append(m)
        return m

    pts = _batch_inputs(32, clouds, stride)
    origins = np.array([gs.batch_origin(name)] * 3, dtype=np.float32)
    _check_batch_against_oracle(seg, clouds, pts, origins, np.full(3, gs.BATCH_BASE_Z), gs.FRAMES, {0, 1, 2}, tag=f"set {name} slot configs",
                                make_ref=make_ref, n_points=shrink)
    assert not nan_equal(refs[0].layer("groundpatch"), refs[2].layer("groundpatch"))
    seg.close()


# ---------------------------------------------------------------- the ignore test at the constant's own float
@pytest.mark.parametrize("name", gs.IGNORE_SETS)
def test_ignore_test_exactly_at_one_float_below_and_above_the_constant(name):
    cloud, origin, special, L, R, vpad, mds = gs.ignore_cloud(name)
    r = run_pair(cloud, length=L, resolution=R, origin=origin, frames=2, geom=(vpad, mds))   # (classes, cells, labels, cloud, layers)
    assert (r["cls"][special["at"]] != oracle.IGNORED).all() and (r["cls"][special["above"]] != oracle.IGNORED).all()
    assert (r["cls"][special["below"]] == oracle.IGNORED).all()
    # ... and through the batched front end (points per wave chunk of a large context)
    B = 3
    clouds = [cloud, cloud[::-1].copy(), cloud[: len(cloud) // 2]]
    stride = (len(cloud) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(L, R, n_slots=B, max_points=stride, vertical_point_ang_dist=vpad, min_dist_squared=mds)
    _check_batch_against_oracle(seg, clouds, _batch_inputs(32, clouds, stride), np.array([origin] * B, dtype=np.float32), np.full(B, -1.73), 2,
                                {0, 1, 2}, tag=f"ignore {name}",
                                make_ref=lambda: oracle.OracleMap(L, R, vertical_point_ang_dist=vpad, min_dist_squared=mds))
    for b, c in enumerate(clouds):
        cls, _ = seg.point_classes(len(c), map=seg.map(b))
        om = oracle.OracleMap(L, R, vertical_point_ang_dist=vpad, min_dist_squared=mds)
        om.stage_reset()
        assert np.array_equal(cls == oracle.IGNORED, om.stage_insert(c, origin)[0] == oracle.IGNORED), b
    seg.close()


# ---------------------------------------------------------------- controls and validation
def test_defaults_written_out_equal_zeros():
    cloud = gs.scaled_cloud(120.0, 3, 400)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=1, max_points=len(cloud)),
            api.GroundSegmentation().init(120.0, 0.33, n_slots=1, max_points=len(cloud), vertical_point_ang_dist=gs.DEFAULT_VPAD,
                                          min_dist_squared=gs.DEFAULT_MDS)]
    ref = oracle.OracleMap(120.0, 0.33)
    assert np.array_equal(segs[0].expected_points(), segs[1].expected_points())
    for frame in range(3):
        r = ref.filter_cloud(cloud, (0.1, 0.2, 0.0), -1.73)
        outs = [s.filter_cloud(cloud, (0.1, 0.2, 0.0), -1.73, return_details=True) for s in segs]
        for out, labels, index in outs:
            assert out.tobytes() == r["out_points"].tobytes() and np.array_equal(labels, r["label"]) and np.array_equal(index, r["index"])
        for s in segs:
            assert_same_state(s.map(0), ref, f"frame {frame}")
    for s in segs:
        s.close()


@pytest.mark.parametrize("field", ["vertical_point_ang_dist", "min_dist_squared"])
@pytest.mark.parametrize("value", [-1.0, -1e-30, float("nan"), float("inf"), float("-inf")])
def test_gg_create_refuses_negative_and_non_finite_constants(field, value):
    L = _lib.load()
    g = _lib.GGGeometry(120.0, 0.33, 0.0, 0.0)
    setattr(g, field, value)
    ctx = C.c_void_p()
    assert L.gg_create(C.byref(g), 1, 64, 0, C.byref(ctx)) == -2   # GG_ERR_GEOMETRY
    assert not ctx.value
    with pytest.raises(api.GroundGridError):
        api.GroundSegmentation().init(120.0, 0.33, n_slots=1, max_points=64, **{field: value})


def test_gg_create_takes_zero_as_the_reference_value():
    L = _lib.load()
    for zero in (0.0, -0.0):
        g = _lib.GGGeometry(120.0, 0.33, zero, zero)
        ctx = C.c_void_p()
        assert L.gg_create(C.byref(g), 1, 64, 0, C.byref(ctx)) == 0 and ctx.value
        buf = np.empty(364 * 364, dtype=np.float32)
        assert L.gg_get_expected_points(ctx, buf.ctypes.data) == 0
        assert np.array_equal(buf.reshape((364, 364), order="F"), oracle.OracleMap(120.0, 0.33).expected_points())
        L.gg_destroy(ctx)
