"""The oracle against the reference's OWN translation unit, compiled (oracle/ref_build.py): src/GroundSegmentation.cpp of the
reference, read where it lies and built unmodified against the functional stand-ins of oracle/ref_shim/, run one process per
scenario (oracle/ref.py).  Every implicit conversion the oracle spells out as a cast is decided here by a C++ compiler.  What this
does not pin: the stand-ins' arithmetic is the project's own restated third-party convention (tools/pin/README.md) -- parity stays
unpinned for those five conventions.

Everything is bit-exact (the returned cloud by its bytes, layers by their uint32 views with a NaN mask: NaN == NaN, -0.0 != 0.0);
there is no tolerance anywhere.

Where the reference is on the machine the tests build and run it, or fail.  They skip only where neither the reference nor
oracle/_ref/gg_ref_run exists; the digest tests (tests/golden/ref_build_digests.json, recorded from the reference build alone by
oracle/ref_record.py) run everywhere and hold the oracle to the recorded reference results.
"""
import numpy as np
import pytest

from oracle import oracle, ref, ref_build
from tests import edge_scenes as es
from tests import geom_sets as gs
from tests import ref_scenes as rs

TIME_LIMIT_S = 120.0   # per reference process; the slowest scene takes well under a second


@pytest.fixture(scope="module")
def reference():
    if ref_build.have_reference():
        ref_build.build()          # a compile error is a failure, not a skip
    elif not ref_build.have_binaries():
        pytest.skip("neither the reference nor oracle/_ref/gg_ref_run is on this machine")
    return ref


def _compare_scene(name, binary=None, eigen_reduction=0, digests=None):
    """'' if every frame of the scene is bit-identical between the reference binary and the oracle, else the first difference;
    `digests`: a list that receives the digests of the reference run's frames"""
    scene = rs.scene(name)
    R = rs.run_reference(scene, binary=binary, time_limit=TIME_LIMIT_S)
    O = rs.run_oracle(scene, eigen_reduction)
    assert len(R) == len(O) == scene.frames
    if digests is not None:
        digests += [rs.frame_digest(out, layers) for out, layers in R]
    for f, ((r_out, r_layers), (o_out, o_layers, _)) in enumerate(zip(R, O)):
        msg = rs.describe_difference(o_out, o_layers, r_out, r_layers, f"{name} frame {f} (oracle != reference)")
        if msg:
            return msg
    return ""


# ---------------------------------------------------------------- the committed golden vectors
@pytest.mark.parametrize("fname", rs.GOLDEN_FILES)
def test_reference_build_reproduces_the_golden_vectors(reference, fname):
    """tests/golden/*.npz were written by the oracle; the reference build reproduces what they record"""
    g = np.load(rs.GOLDEN + "/" + fname)
    scene = rs.golden_scene(fname)
    R = rs.run_reference(scene, time_limit=TIME_LIMIT_S)
    raw = rs.cloud_bytes(scene.cloud)
    for f, (out, layers) in enumerate(R):
        label, index = g[f"label_{f}"], g[f"index_{f}"]
        want = np.zeros((int((index >= 0).sum()), 32), np.uint8)
        want[index[index >= 0]] = raw[index >= 0]
        want.view(np.float32).reshape(-1, 8)[index[index >= 0], 4] = label[index >= 0].astype(np.float32)
        assert out.shape == want.shape, (fname, f)
        bad = np.flatnonzero((out != want).any(axis=1))
        assert len(bad) == 0, f"{fname} frame {f}: returned cloud differs at positions {bad[:5]}"
        for layer in ("ground", "groundpatch", "variance"):
            a, b = rs.canonical_bits(layers[layer]), rs.canonical_bits(g[f"{layer}_{f}"])
            assert np.array_equal(a, b), f"{fname} frame {f}: layer {layer} differs at {np.argwhere(a != b)[:3].tolist()}"


def test_golden_file_list_is_complete():
    import os

    assert sorted(f for f in os.listdir(rs.GOLDEN) if f.endswith(".npz")) == sorted(rs.GOLDEN_FILES)


# ---------------------------------------------------------------- whole filter_cloud calls, every scene, every frame
@pytest.mark.parametrize("name", rs.names())
def test_oracle_matches_the_reference_build(reference, name):
    """returned cloud (labels 49 / 99, order, bytes) and all 11 layers after every frame; and this fresh run of the reference build
    reproduces the recorded digests (a mismatch with the arrays equal means the file is stale: re-run oracle/ref_record.py)"""
    fresh = []
    msg = _compare_scene(name, digests=fresh)
    assert not msg, msg
    assert fresh == rs.load_digests()["scenes"][name]["frames"], \
        f"{name}: a fresh reference run equals the oracle but not tests/golden/ref_build_digests.json: the file is stale"


def test_exclusions_are_named_and_few():
    """a scene is left out only where the reference has no defined, terminating behaviour: by name, with its reason, at most 2 of the
    adversarial scenes; every other scene of the catalogue is compared (and recorded)"""
    adversarial = rs.names("adversarial/", excluded=True)
    assert len(adversarial) == len(es.adversarial_scenes())
    assert set(rs.EXCLUDED) <= set(rs.names(excluded=True))
    assert all(isinstance(r, str) and len(r) > 40 for r in rs.EXCLUDED.values())
    assert len([n for n in rs.EXCLUDED if n.startswith("adversarial/")]) <= 2
    assert len(rs.EXCLUDED) <= 2
    assert set(rs.names()) == set(rs.names(excluded=True)) - set(rs.EXCLUDED)
    assert set(rs.load_digests()["scenes"]) == set(rs.names())
    assert {f"label_tolerance/{'_'.join(f'{v:g}' for v in c)}" for c in es.LABEL_TOLERANCE_CONFIGS} <= set(rs.names())
    assert {f"sized/{n}" for n in es.BATCH_SIZES} <= set(rs.names())
    assert {g[3] for g in rs.GEOMETRIES} >= {64, 67, 20, 364, 1000}


@pytest.mark.parametrize("g", rs.GEOMETRIES, ids=[g[0] for g in rs.GEOMETRIES])
def test_geometries_have_the_cell_counts_they_are_named_for(g):
    m = oracle.OracleMap(g[1], g[2], pos=g[4])
    assert m.rows == m.cols == g[3]


# ---------------------------------------------------------------- configuration
@pytest.mark.parametrize("field,value", rs.CONFIG_EDITS)
def test_every_config_field_changes_the_recorded_reference_result(field, value):
    """each field off its default reaches the reference's result (recorded digests against the default run's)"""
    d = rs.load_digests()["scenes"]
    base, moved = d["config/default"]["frames"], d[rs.config_name(field, value)]["frames"]
    assert base[-1] != moved[-1], f"{field} = {value} changes nothing"
    assert any(base[-1][k] != moved[-1][k] for k in ("labels", "ground", "groundpatch")), (field, value)


def test_config_edits_cover_every_field_and_both_sides_of_the_thresholds():
    fields = {f for f, _ in rs.CONFIG_EDITS} | {f for f, _ in rs.CONFIG_UNUSED} | {"thread_count"}
    assert fields == {n for n, _ in oracle.Config._fields_}
    decay = sorted(v for f, v in rs.CONFIG_EDITS if f == "occupied_cells_decrease_factor")
    assert decay[0] < 1.25 < decay[-1]
    # point_count_cell_variance_threshold on both sides of the cells' counts: some cell of the scene holds more than 1 and none 100000
    scene = rs.config_scene()
    m = oracle.OracleMap(scene.length, scene.resolution)
    m.stage_reset()
    m.stage_insert(scene.cloud, scene.origin)
    counts = m.layer("points")
    thresholds = sorted(v for f, v in rs.CONFIG_EDITS if f == "point_count_cell_variance_threshold")
    assert thresholds[0] < counts.max() < thresholds[-1] and (counts >= 10).any() and ((counts > 0) & (counts < 10)).any()
    rings = scene.cloud["ring"]
    max_ring = [v for f, v in rs.CONFIG_EDITS if f == "max_ring"][0]
    assert (rings > max_ring).any() and (rings <= max_ring).any()
    d = rs.load_digests()["scenes"]
    for field, value in rs.CONFIG_UNUSED:   # never read by the path: the recorded result is the default's
        assert d[rs.config_name(field, value)]["frames"] == d["config/default"]["frames"]


# ---------------------------------------------------------------- insert_cloud's three lists
def _insert_state(scene, warm_frames):
    """an oracle map after `warm_frames` frames and the filter_cloud prologue (:61-75): the layers insert_cloud starts from"""
    vpad, mds = gs.scene_constants(scene)
    m = oracle.OracleMap(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z, vertical_point_ang_dist=vpad, min_dist_squared=mds)
    if scene.cfg_edit:
        scene.cfg_edit(m.cfg)
    for f in range(warm_frames):
        m.filter_cloud(gs.frame_cloud(scene, f), scene.origin, scene.base_z)
    m.stage_reset()
    return m


INSERT_SCENES = [n for n in rs.names() if not n.startswith(("config/", "golden/", "sized/"))] + ["config/default", "config/max_ring=31",
                                                                                                 "golden/micro_64_stateful"]


@pytest.mark.parametrize("name", INSERT_SCENES)
def test_insert_cloud_lists_and_cells(reference, name):
    """insert_cloud(0, n) on a cold and on a warm map: the kept / ignored / outlier lists with their cells, and the layers it wrote"""
    scene = rs.scene(name)
    for warm in sorted({0, scene.frames - 1}):
        m = _insert_state(scene, warm)
        sc = ref.Scenario(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z, cfg=ref.single_thread(m.cfg), layers=m.layers_copy())
        sc.insert_cloud(scene.cloud, scene.origin)
        (r,) = ref.run(sc, binary=rs.variant_of(scene), time_limit=TIME_LIMIT_S)
        cls, cell = m.stage_insert(scene.cloud, scene.origin)
        for kind, code in (("kept", oracle.KEPT), ("ignored", oracle.IGNORED)):
            idx = np.flatnonzero(cls == code)
            got = r[kind]
            assert np.array_equal(got["i"], idx.astype(np.uint64)), f"{name} warm {warm}: {kind} list differs"
            assert np.array_equal(got["row"] + got["col"] * m.rows, cell[idx]), f"{name} warm {warm}: cells of the {kind} list differ"
        assert np.array_equal(r["outliers"], np.flatnonzero(cls == oracle.OUTLIER).astype(np.uint64)), f"{name} warm {warm}: outliers"
        msg = rs.describe_difference(np.zeros((0, 32), np.uint8), m.layers_copy(), np.zeros((0, 32), np.uint8), r["layers"], f"{name} warm {warm}")
        assert not msg, msg


def test_insert_cloud_sub_ranges(reference):
    """insert_cloud(start, end) on parts of the cloud, one after the other on the same map, as the reference's threads would split it"""
    scene = rs.scene("random/2")
    m = _insert_state(scene, 1)
    n = len(scene.cloud)
    cuts = [0, 1, n // 3, n // 3, n - 1, n]
    sc = ref.Scenario(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z, cfg=ref.single_thread(m.cfg), layers=m.layers_copy())
    for a, b in zip(cuts[:-1], cuts[1:]):
        sc.insert_cloud(scene.cloud, scene.origin, start=a, end=b, dump=(b == n))
    rr = ref.run(sc, time_limit=TIME_LIMIT_S)
    cls, cell = m.stage_insert(scene.cloud, scene.origin)
    for kind, code in (("kept", oracle.KEPT), ("ignored", oracle.IGNORED)):   # the parts' lists, joined in call order, with their cells
        got = np.concatenate([r[kind] for r in rr])
        idx = np.flatnonzero(cls == code)
        assert len(idx) > 0, f"random/2 has no {kind} point"
        assert np.array_equal(got["i"], idx.astype(np.uint64)), f"sub-ranges: {kind} list differs"
        assert np.array_equal(got["row"] + got["col"] * m.rows, cell[idx]), f"sub-ranges: cells of the {kind} list differ"
    for r, (a, b) in zip(rr, zip(cuts[:-1], cuts[1:])):   # every call appended points of its own range only
        for kind in ("kept", "ignored"):
            assert ((r[kind]["i"] >= a) & (r[kind]["i"] < b)).all()
        assert ((r["outliers"] >= a) & (r["outliers"] < b)).all()
    assert np.array_equal(np.concatenate([r["outliers"] for r in rr]), np.flatnonzero(cls == oracle.OUTLIER).astype(np.uint64))
    msg = rs.describe_difference(np.zeros((0, 32), np.uint8), m.layers_copy(), np.zeros((0, 32), np.uint8), rr[-1]["layers"], "sub-ranges")
    assert not msg, msg


def test_scenario_refuses_more_than_one_thread():
    """the reference is deterministic at thread_count = 1 only: a scenario with the default 8 is an error, not a silent 1"""
    c = oracle.default_config()
    assert c.thread_count != 1
    with pytest.raises(ValueError):
        ref.Scenario(120.0, 0.33, cfg=c)
    one = ref.single_thread(c)
    assert one.thread_count == 1 and one.max_ring == c.max_ring and one.outlier_tolerance == c.outlier_tolerance


# ---------------------------------------------------------------- the stage members one by one, on foreign layers
def _foreign_layers(n, seed):
    """random finite layers of an n x n map, plus a NaN cell and an inf cell in the layers the stages read"""
    rng = np.random.default_rng(seed)
    lay = {
        "points": np.where(rng.random((n, n)) < 0.7, rng.integers(0, 40, (n, n)), 0).astype(np.float32) + (rng.random((n, n)) < 0.05) * np.float32(0.5),
        "ground": rng.normal(-1.7, 0.3, (n, n)),
        "groundpatch": np.where(rng.random((n, n)) < 0.5, rng.uniform(0, 1, (n, n)), rng.uniform(0, 1e-3, (n, n))),
        "minGroundHeight": rng.normal(-1.8, 0.2, (n, n)),
        "maxGroundHeight": rng.normal(-1.2, 0.2, (n, n)),
        "groundCandidates": rng.normal(-1.7, 0.1, (n, n)),
        "planeDist": rng.normal(-1.7, 0.1, (n, n)),
        "m2": rng.uniform(0, 1, (n, n)) * 10.0 ** rng.integers(-9, 1, (n, n)),
        "meanVariance": rng.normal(-1.7, 0.1, (n, n)),
        "pointsRaw": rng.integers(0, 50, (n, n)),
        "variance": rng.uniform(0, 1e-3, (n, n)) * 10.0 ** rng.integers(-6, 1, (n, n)),
    }
    lay = {k: np.asfortranarray(v, dtype=np.float32) for k, v in lay.items()}
    for name in ("ground", "groundpatch", "minGroundHeight", "m2", "variance"):
        lay[name][n // 3, n // 4] = np.nan
        lay[name][n // 2 + 3, n // 2 - 5] = np.inf
    lay["minGroundHeight"][n // 4, n // 3] = -np.inf
    return lay


def _oracle_with(length, resolution, lay, pos=(0.0, 0.0)):
    m = oracle.OracleMap(length, resolution, pos=pos)
    for k, v in lay.items():
        m.set_layer(k, v)
    return m


def _assert_layers(m, r, what):
    msg = rs.describe_difference(np.zeros((0, 32), np.uint8), m.layers_copy(), np.zeros((0, 32), np.uint8), r["layers"], what)
    assert not msg, msg


STAGE_GEOMETRIES = [(21.12, 0.33, 64), (22.0, 0.33, 67), (4.0, 0.2, 20), (120.0, 0.33, 364)]


@pytest.mark.parametrize("length,resolution,n", STAGE_GEOMETRIES)
def test_detect_ground_patches_quadrant_by_quadrant(reference, length, resolution, n):
    lay = _foreign_layers(n, 100 + n)
    for section in range(4):   # each quadrant alone on the same foreign layers, then all four in a row
        m = _oracle_with(length, resolution, lay)
        assert m.rows == n
        (r,) = ref.run(ref.Scenario(length, resolution, layers=lay).detect_ground_patches(section), time_limit=TIME_LIMIT_S)
        m.stage_detect_section(section)
        _assert_layers(m, r, f"{n} cells, detect_ground_patches({section})")
        assert not rs.same_bits(m.layer("ground"), lay["ground"]) or n == 20, "the quadrant changed nothing"
    m = _oracle_with(length, resolution, lay)
    sc = ref.Scenario(length, resolution, layers=lay)
    for section in (3, 1, 0, 2):
        sc.detect_ground_patches(section)
        m.stage_detect_section(section)
    _assert_layers(m, ref.run(sc, time_limit=TIME_LIMIT_S)[-1], f"{n} cells, the four quadrants")


@pytest.mark.parametrize("length,resolution,n", STAGE_GEOMETRIES)
def test_spiral_ground_interpolation_on_foreign_layers(reference, length, resolution, n):
    lay = _foreign_layers(n, 200 + n)
    m = _oracle_with(length, resolution, lay)
    # (a rotated base transform: the zero point's image is the translation whatever the rotation)
    sc = ref.Scenario(length, resolution, layers=lay, quaternion=(0.1, -0.2, 0.3, 0.9273618495495703))
    (r,) = ref.run(sc.spiral_ground_interpolation(-1.625), time_limit=TIME_LIMIT_S)
    m.stage_spiral(-1.625)
    _assert_layers(m, r, f"{n} cells, spiral_ground_interpolation")


@pytest.mark.parametrize("length,resolution,n", STAGE_GEOMETRIES[:3])
def test_detect_ground_patch_and_interpolate_cell_one_by_one(reference, length, resolution, n):
    """detect_ground_patch<3> / <5>(i, j) and interpolate_cell(x, y) on single cells: the corners the loops reach, the map centre,
    the cells around the NaN and the inf cell, random ones"""
    lay = _foreign_layers(n, 300 + n)
    rng = np.random.default_rng(n)
    cells = [(2, 2), (n - 3, n - 3), (2, n - 3), (n // 2, n // 2), (n // 2 - 1, n // 2 - 1), (n // 3, n // 4), (n // 3 + 1, n // 4 - 1),
             (n // 2 + 3, n // 2 - 5), (n // 2 + 2, n // 2 - 4), (n // 4, n // 3)]
    cells += [tuple(int(v) for v in rng.integers(2, n - 2, 2)) for _ in range(30)]
    m = _oracle_with(length, resolution, lay)
    sc = ref.Scenario(length, resolution, layers=lay)
    for k, (i, j) in enumerate(cells):
        S = 3 if k % 2 else 5
        sc.detect_ground_patch(S, i, j, dump=False)
        m.detect_ground_patch(S, i, j)
    changed = not rs.same_bits(m.layer("ground"), lay["ground"])
    visits = [(1, 1), (n - 2, n - 2), (1, n - 2)] + cells
    for k, (x, y) in enumerate(visits):
        sc.interpolate_cell(x, y, dump=(k == len(visits) - 1))
        m.interpolate_cell(x, y)
    _assert_layers(m, ref.run(sc, time_limit=TIME_LIMIT_S)[-1], f"{n} cells, single cells")
    assert changed, "no detect_ground_patch call changed the terrain"


@pytest.mark.parametrize("length,resolution,n", STAGE_GEOMETRIES + [(200.0, 0.2, 1000)])
def test_init_expected_points(reference, length, resolution, n):
    (r,) = ref.run(ref.Scenario(length, resolution).init(), time_limit=TIME_LIMIT_S)
    m = oracle.OracleMap(length, resolution)
    assert (r["rows"], r["cols"]) == (m.rows, m.cols) == (n, n)
    a, b = m.expected_points().view(np.uint32), r["expected_points"].view(np.uint32)
    assert np.array_equal(a, b), f"expectedPoints differs at {np.argwhere(a != b)[:3].tolist()}"


# ---------------------------------------------------------------- the two compile-time constants at other values (constant sets A and B)
def test_variant_scenes_are_in_the_catalogue_with_their_constants():
    """every geom/ scene is compared and recorded (none excluded), and the binary it runs through was compiled with its pair"""
    geom = rs.names("geom/", excluded=True)
    assert sorted(geom) == sorted(f"geom/{n}{k}" for n in rs.GEOM_VARIANTS for k in ("", "_ignore")) and not set(geom) & set(rs.EXCLUDED)
    assert set(geom) <= set(rs.load_digests()["scenes"])
    for n, variant in rs.GEOM_VARIANTS.items():
        L, R, vpad, mds = gs.geometry(n)
        assert [np.float32(v) for v in ref_build.VARIANTS[variant]] == [np.float32(vpad), np.float32(mds)]
        assert np.float32(vpad) != np.float32(gs.DEFAULT_VPAD) and np.float32(mds) != np.float32(gs.DEFAULT_MDS)
        for k in ("", "_ignore"):
            sc = rs.scene(f"geom/{n}{k}")
            assert gs.scene_constants(sc) == (vpad, mds) and rs.variant_of(sc) == variant and (sc.length, sc.resolution) == (L, R)


def test_variant_header_differs_from_the_reference_header_in_two_initialisers(reference):
    """the shadow header of a variant is the reference's header with the two initialisers replaced: exactly two lines differ, one names each
    member, and what stands there is the set's float"""
    if not ref_build.have_reference():
        pytest.skip("the reference is not on this machine (its binaries travelled here): nothing to shadow")
    with open(ref_build.reference_header()) as f:
        original = f.read().split("\n")
    for variant, pair in ref_build.VARIANTS.items():
        with open(ref_build.write_shadow_header(variant) + "/groundgrid/GroundSegmentation.h") as f:
            shadow = f.read().split("\n")
        assert len(shadow) == len(original)
        diff = [(a, b) for a, b in zip(original, shadow) if a != b]
        assert len(diff) == 2
        for (a, b), member, value in zip(diff, ref_build._MEMBERS, pair):
            assert member in a and member in b
            assert np.float32(float.fromhex(b.split("=")[1].split(";")[0].strip().rstrip("f"))) == np.float32(value)


def test_variant_constants_reach_the_reference_result():
    """recorded digests: the terrain of geom/A and geom/B is not what the same scene leaves at the default constants (oracle, here)"""
    d = rs.load_digests()["scenes"]
    for n in rs.GEOM_VARIANTS:
        sc = rs.scene(f"geom/{n}")
        plain = es.Scene(sc.name, sc.cloud, sc.branch, length=sc.length, resolution=sc.resolution, origin=sc.origin, base_z=sc.base_z,
                         frames=sc.frames, extra={"frame_points": sc.extra["frame_points"]})
        last = rs.run_oracle(plain)[-1]
        got = rs.frame_digest(last[0], last[1])
        rec = d[f"geom/{n}"]["frames"][-1]
        assert all(got[k] != rec[k] for k in ("ground", "groundpatch", "labels")), n


# ---------------------------------------------------------------- the comparison can see one convention apart
SENSITIVITY_SCENE = "label_tolerance/0.0005_0.3_0.1"


def test_comparison_sees_the_eigen_reduction_order(reference):
    """the reference built with the Eigen 3.4 + SSE order of the 5x5 block sums against the oracle left at GG_EIGEN_33: they DIFFER
    (sums that round differently, some by one ulp, reach the terrain); against the oracle at GG_EIGEN_34_SSE: bit-identical"""
    msg = _compare_scene(SENSITIVITY_SCENE, binary="gg_ref_run_eigen34", eigen_reduction=0)
    assert msg, "the Eigen 3.4 binary and the Eigen 3.3 oracle agree: the comparison cannot see a reduction order"
    assert "layer ground" in msg or "layer groundpatch" in msg or "returned cloud" in msg, msg
    msg = _compare_scene(SENSITIVITY_SCENE, binary="gg_ref_run_eigen34", eigen_reduction=1)
    assert not msg, msg
    scene = rs.scene(SENSITIVITY_SCENE)
    a = rs.run_reference(scene, binary="gg_ref_run_eigen34", time_limit=TIME_LIMIT_S)[-1][1]["ground"].view(np.uint32)
    b = rs.run_reference(scene, binary="gg_ref_run", time_limit=TIME_LIMIT_S)[-1][1]["ground"].view(np.uint32)
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    print(f"{SENSITIVITY_SCENE}: {int((d > 0).sum())} terrain cells differ between the two orders, {int((d == 1).sum())} of them by one ulp")
    assert (d > 0).sum() >= 100 and (d == 1).sum() >= 1


# ---------------------------------------------------------------- the recorded digests
@pytest.mark.parametrize("name", rs.names())
def test_oracle_reproduces_the_recorded_reference_digests(name):
    """runs everywhere: a checkout without the reference is still held to what the reference build returned"""
    rec = rs.load_digests()["scenes"][name]
    scene = rs.scene(name)
    assert rs.input_digest(scene) == rec["input"] and len(scene.cloud) == rec["points"], \
        f"{name}: the scene generator drifted (its inputs are not those the digests were recorded from): re-run oracle/ref_record.py"
    O = rs.run_oracle(scene)
    assert len(O) == len(rec["frames"])
    for f, (out, layers, _) in enumerate(O):
        got = rs.frame_digest(out, layers)
        bad = [k for k in rec["frames"][f] if got[k] != rec["frames"][f][k]]
        assert not bad, f"{name} frame {f}: the oracle does not reproduce the reference build's {bad}"


def test_digest_file_names_the_exclusions_and_conventions():
    rec = rs.load_digests()
    assert rec["excluded"] == rs.EXCLUDED
    assert rec["conventions"] == {"eigen": "GG_EIGEN_33", "rotation": "kdl"}
