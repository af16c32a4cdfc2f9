"""The scenes on which the oracle -- and, through the recorded digests, the HIP path -- is held to the reference's own translation
unit compiled against stand-ins (oracle/ref_build.py).  A plain helper module shared by oracle/ref_record.py (which
writes tests/golden/ref_build_digests.json from the reference binary alone), tests/test_reference_build_cpu.py and
tests/test_reference_vectors_gpu.py.  The product never imports it, and nothing here reads the reference.

A scene is an edge_scenes.Scene: the same cloud for `frames` consecutive filter_cloud calls on one map (the geom/ scenes: a shorter
prefix of it in every frame, tests/geom_sets.py).  Every generator is seeded.

The geom/ scenes carry a pair of the reference's two compile-time constants (include/groundgrid/GroundSegmentation.h:69-70) in
Scene.extra; run_reference runs them through the variant binary compiled with that pair (oracle/ref_build.py VARIANTS).
"""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

from groundgrid_amd import synth
from tests import edge_scenes as es
from tests import geom_sets as gs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DIGESTS = os.path.join(GOLDEN, "ref_build_digests.json")
LAYERS = ["points", "ground", "groundpatch", "minGroundHeight", "maxGroundHeight", "groundCandidates", "planeDist", "m2",
          "meanVariance", "pointsRaw", "variance"]
FUZZ_SEEDS = range(6)   # the seeds of tests/test_gpu_parity.py::test_random_scenes_fuzz

# Scenes on which the REFERENCE has no defined, terminating behaviour: they are left out of the comparison by name.  Nothing else
# may be excluded, and at most 2 of the adversarial scenes (tests/test_reference_build_cpu.py asserts both).
EXCLUDED = {
    "adversarial/corrupt_z": "the line-of-sight walk of src/GroundSegmentation.cpp:258 has no bound: for z = -1e9 ... -3e38 `int step` counts "
                             "past 2^31 (signed overflow, undefined); the project bounds the walk as a documented deviation (GGO_WALK_MAX_STEP)",
}


def golden_scene(fname) -> es.Scene:
    """the inputs of a committed tests/golden/*.npz (its recorded outputs are compared by the tests themselves)"""
    g = np.load(os.path.join(GOLDEN, fname))
    cloud = np.frombuffer(g["cloud"].tobytes(), dtype=synth.POINT_DTYPE)
    return es.Scene(fname[:-4], cloud, "golden vector", length=float(g["length"]), resolution=float(g["resolution"]),
                    pos=tuple(float(v) for v in g["pos"]), origin=tuple(float(v) for v in g["origin"]), base_z=float(g["base_z"]),
                    frames=int(g["frames"]))


GOLDEN_FILES = ["edge_cases_64.npz", "hdl64_small_364.npz", "micro_64_stateful.npz", "random_364_moved.npz"]

# ---------------------------------------------------------------- geometries: even and odd cell counts, a moved map
# (:38, :325-328 and :403 all divide the size by two)
GEOMETRIES = [
    # name, length, resolution, cells, map position, sensor origin, points, extent of the cloud, frames
    ("cells64_moved", 21.12, 0.33, 64, (1.3, -2.1), (0.4, -0.3, 0.2), 9000, 12.0, 3),
    ("cells67_odd", 22.0, 0.33, 67, (0.0, 0.0), (0.5, 0.25, 0.1), 9000, 12.5, 3),
    ("cells67_odd_moved", 22.0, 0.33, 67, (-7.77, 12.21), (-7.0, 12.0, 0.0), 9000, 12.5, 2),
    ("cells20", 4.0, 0.2, 20, (0.0, 0.0), (4.5, 0.5, 0.3), 3000, 2.4, 3),
    ("cells364_moved", 120.0, 0.33, 364, (4.29, -2.64), (4.0, -2.5, 0.1), 20000, 66.0, 2),
    ("cells1000_sparse", 200.0, 0.2, 1000, (0.7, 0.3), (0.0, 0.0, 0.0), 4000, 104.0, 2),
]


def geometry_scene(name, length, resolution, cells, pos, origin, n, extent, frames) -> es.Scene:
    c = synth.random_cloud(n, seed=9000 + cells + n, extent=extent)
    c["x"] = (c["x"].astype(np.float64) + pos[0]).astype(np.float32)
    c["y"] = (c["y"].astype(np.float64) + pos[1]).astype(np.float32)
    return es.Scene(name, c, "index maths that halves the size", length=length, resolution=resolution, pos=pos, origin=origin, base_z=-1.6,
                    odom_z=0.1, frames=frames, extra={"cells": cells})


# ---------------------------------------------------------------- configuration: every field moved off its default
@functools.lru_cache(maxsize=None)
def config_base_cloud():
    """a sensor cloud with one point in five under the surface (line-of-sight candidates), seen from off the map centre"""
    return es.line_of_sight_clouds()[1]


# (field, value): every field of gg_config that the path reads, moved so that the result of CONFIG_FRAMES frames changes;
# occupied_cells_decrease_factor on both sides of 1.25, point_count_cell_variance_threshold on both sides of the cells' counts
# (the densest cells of the cloud hold tens of points, the default is 10)
CONFIG_EDITS = [
    ("point_count_cell_variance_threshold", 1),
    ("point_count_cell_variance_threshold", 100000),
    ("max_ring", 31),
    ("distance_factor", 0.01),
    ("minimum_distance_factor", 0.005),
    ("miminum_point_height_threshold", 0.5),
    ("minimum_point_height_obstacle_threshold", 0.25),
    ("outlier_tolerance", 0.3),
    ("ground_patch_detection_minimum_point_count_threshold", 0.6),
    ("patch_size_change_distance", 8.0),
    ("occupied_cells_decrease_factor", 1.1),
    ("occupied_cells_decrease_factor", 7.3),
    ("occupied_cells_point_count_factor", 7.0),
    ("min_outlier_detection_ground_confidence", 0.3),
    ("min_outlier_detection_ground_confidence", 4.0),
]
# read by nothing on the path (src/GroundSegmentation.cpp never names it): moving it must change nothing
CONFIG_UNUSED = [("groundpatch_detection_minimum_threshold", 0.5)]
# thread_count is not varied: the reference is deterministic only at 1 (its insertion threads race on shared cells, :101-106)
CONFIG_FRAMES = 3


def config_edit(field, value):
    def edit(c):
        setattr(c, field, value)
    return edit


def config_name(field, value) -> str:
    return f"config/{field}={value:g}"


def config_scene(field=None, value=None) -> es.Scene:
    name = "config/default" if field is None else config_name(field, value)
    return es.Scene(name, config_base_cloud(), "a configuration field off its default", origin=(7.5, -3.0, 0.4), frames=CONFIG_FRAMES,
                    cfg_edit=None if field is None else config_edit(field, value))


# ---------------------------------------------------------------- the two sensor constants off their defaults (constant sets A and B)
GEOM_VARIANTS = {"A": "gg_ref_run_geomA", "B": "gg_ref_run_geomB"}   # set -> the reference binary compiled with its pair


def geom_scene(name) -> es.Scene:
    """the shrinking-cloud scene of a constant set, as the GPU file runs it"""
    sc = gs.scene(name)
    return es.Scene(sc.name, sc.cloud, sc.branch, length=sc.length, resolution=sc.resolution, origin=sc.origin, base_z=sc.base_z,
                    frames=sc.frames, extra={**sc.extra, "variant": GEOM_VARIANTS[name]})


def geom_ignore_scene(name) -> es.Scene:
    """the set's ignore-test cloud (points whose squared distance is exactly the constant, the float below and the float above)"""
    cloud, origin, _, L, R, vpad, mds = gs.ignore_cloud(name)
    return es.Scene(f"geom/{name}_ignore", cloud, "the ignore test of :237 at the constant's own float", length=L, resolution=R, origin=origin,
                    frames=2, extra={"vertical_point_ang_dist": vpad, "min_dist_squared": mds, "variant": GEOM_VARIANTS[name]})


def variant_of(scene) -> str:
    return scene.extra.get("variant", "gg_ref_run")


# ---------------------------------------------------------------- the catalogue
@functools.lru_cache(maxsize=None)
def _adversarial():
    return {"adversarial/" + s.name: s for s in es.adversarial_scenes()}


@functools.lru_cache(maxsize=None)
def builders() -> dict:
    """name -> function that builds the Scene, in a fixed order; the excluded scenes are in it (callers skip them by EXCLUDED)"""
    out = {}
    for f in GOLDEN_FILES:
        out["golden/" + f[:-4]] = functools.partial(golden_scene, f)
    for name in _adversarial():
        out[name] = functools.partial(_adversarial().__getitem__, name)
    for cfg in es.LABEL_TOLERANCE_CONFIGS:
        out["label_tolerance/" + "_".join(f"{v:g}" for v in cfg)] = functools.partial(es.label_tolerance, *cfg)
    for seed in FUZZ_SEEDS:
        out[f"random/{seed}"] = functools.partial(es.random_scene, seed)
    for n in es.BATCH_SIZES:
        out[f"sized/{n}"] = functools.partial(es.sized, n)
    for g in GEOMETRIES:
        out["geometry/" + g[0]] = functools.partial(geometry_scene, *g)
    out["config/default"] = config_scene
    for field, value in CONFIG_EDITS + CONFIG_UNUSED:
        out[config_name(field, value)] = functools.partial(config_scene, field, value)
    for name in GEOM_VARIANTS:
        out["geom/" + name] = functools.partial(geom_scene, name)
        out[f"geom/{name}_ignore"] = functools.partial(geom_ignore_scene, name)
    return out


def scene(name) -> es.Scene:
    return builders()[name]()


def names(prefix=None, excluded=False):
    """the catalogue's names; those of EXCLUDED only when asked for"""
    return [n for n in builders() if (prefix is None or n.startswith(prefix)) and (excluded or n not in EXCLUDED)]


# ---------------------------------------------------------------- digests
def sha(data) -> str:
    """SHA-256 of the bytes, first 16 hex digits (64 bits: the file stays small, a chance match is out of the question)"""
    return hashlib.sha256(bytes(data)).hexdigest()[:16]


def cloud_bytes(cloud) -> np.ndarray:
    return np.frombuffer(np.ascontiguousarray(cloud).tobytes(), dtype=np.uint8).reshape(-1, 32)


def input_digest(scene) -> str:
    """everything a run depends on except the configuration edit (which the scene's name carries)"""
    head = json.dumps([float(np.float32(scene.length)), float(np.float32(scene.resolution)), [float(v) for v in scene.pos],
                       [float(np.float32(v)) for v in scene.origin], float(scene.base_z), float(np.float32(scene.odom_z)), int(scene.frames)])
    if "variant" in scene.extra:   # (only the scenes that carry constants: every older scene keeps its recorded digest)
        head += json.dumps([float(np.float32(v)) for v in gs.scene_constants(scene)] + [scene.extra.get("frame_points")])
    return sha(head.encode() + cloud_bytes(scene.cloud).tobytes())


def canonical_bits(layer) -> np.ndarray:
    """the layer's bits (column-major) with every NaN replaced by one pattern: which NaN an operation leaves -- x86 hands on its first
    NaN operand and makes a negative one for an invalid operation, a GPU makes a positive one -- is decided by the operand order a
    compiler picked, not by the source text.  Everything else keeps its bits: -0.0 != 0.0."""
    a = np.array(layer, dtype=np.float32, order="F")
    bits = a.view(np.uint32)
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def frame_digest(out_points, layers) -> dict:
    """out_points: the returned cloud as (n, 32) bytes; layers: name -> (rows, cols) float32.  `labels` = the intensities in
    returned order, `order` = the returned records with the intensity blanked, `cloud` = all of it."""
    o = np.array(out_points, dtype=np.uint8).reshape(-1, 32)
    blank = o.copy()
    blank[:, 16:20] = 0
    d = {"n": int(o.shape[0]), "labels": sha(o[:, 16:20].tobytes()), "order": sha(blank.tobytes()), "cloud": sha(o.tobytes())}
    for name in LAYERS:
        d[name] = sha(canonical_bits(layers[name]).tobytes(order="F"))
    return d


def pack_frames(frames) -> list:
    """how the file stores a scene's frames: the first in full, every later one as the entries that differ from the frame before"""
    return [f if k == 0 else {key: v for key, v in f.items() if frames[k - 1][key] != v} for k, f in enumerate(frames)]


def unpack_frames(packed) -> list:
    out = []
    for k, f in enumerate(packed):
        out.append(dict(f) if k == 0 else {**out[-1], **f})
    return out


@functools.lru_cache(maxsize=None)
def load_digests() -> dict:
    """the recorded digests with every frame in full (read-only: the result is shared)"""
    with open(DIGESTS) as f:
        doc = json.load(f)
    for s in doc["scenes"].values():
        s["frames"] = unpack_frames(s["frames"])
    return doc


def dump_digests(doc, path=DIGESTS):
    """one line per frame, later frames as differences (pack_frames)"""
    lines = ["{", f'"what": {json.dumps(doc["what"])},', f'"conventions": {json.dumps(doc["conventions"])},',
             f'"excluded": {json.dumps(doc["excluded"])},', '"scenes": {']
    names_ = list(doc["scenes"])
    for n in names_:
        s = doc["scenes"][n]
        lines.append(f'{json.dumps(n)}: {{"input": {json.dumps(s["input"])}, "points": {s["points"]}, "frames": [')
        packed = pack_frames(s["frames"])
        lines += [json.dumps(f) + ("," if k < len(packed) - 1 else "") for k, f in enumerate(packed)]
        lines.append("]}" + ("," if n != names_[-1] else ""))
    lines += ["}", "}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------- the two CPU sides
def run_reference(scene, binary=None, time_limit=None):
    """the scene through the reference binary (default: the one compiled with the scene's constants): one process, `frames` filter_cloud
    steps; returns [(out_points bytes, layers)]"""
    from oracle import ref, ref_build

    binary = binary or variant_of(scene)
    want = ref_build.VARIANTS.get(binary, (0.0, 0.0))
    have = gs.scene_constants(scene)
    assert [np.float32(v) for v in want] == [np.float32(v) for v in have], f"{scene.name}: {binary} was compiled with {want}, the scene asks for {have}"

    cfg = ref.default_config()
    if scene.cfg_edit:
        scene.cfg_edit(cfg)
    sc = ref.Scenario(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z, cfg=cfg)
    for f in range(scene.frames):
        sc.filter_cloud(gs.frame_cloud(scene, f), scene.origin, scene.base_z)
    rs = ref.run(sc, binary=binary, time_limit=time_limit or ref.TIME_LIMIT_S)
    return [(r["out_points"], r["layers"]) for r in rs]


def run_oracle(scene, eigen_reduction=0):
    """the scene through the C oracle; returns [(out_points bytes, layers, result dict)]"""
    from oracle import oracle

    oracle.set_eigen_reduction(eigen_reduction)
    try:
        vpad, mds = gs.scene_constants(scene)
        m = oracle.OracleMap(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z, vertical_point_ang_dist=vpad, min_dist_squared=mds)
        if scene.cfg_edit:
            scene.cfg_edit(m.cfg)
        out = []
        for f in range(scene.frames):
            r = m.filter_cloud(gs.frame_cloud(scene, f), scene.origin, scene.base_z)
            out.append((cloud_bytes(r["out_points"]), m.layers_copy(), r))
        return out
    finally:
        oracle.set_eigen_reduction(0)


def same_bits(a, b) -> bool:
    """bit-exact: NaN == NaN, -0.0 != 0.0"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(canonical_bits(a), canonical_bits(b))


def describe_difference(got_out, got_layers, want_out, want_layers, what="") -> str:
    """'' if the frame is bit-identical (returned cloud: bytes; layers: bits, NaN == NaN), else a line naming the first differing record / layer and cell"""
    g, w = np.asarray(got_out).reshape(-1, 32), np.asarray(want_out).reshape(-1, 32)
    if g.shape != w.shape:
        return f"{what}: returned cloud has {g.shape[0]} points, expected {w.shape[0]}"
    bad = np.flatnonzero((g != w).any(axis=1))
    if len(bad):
        k = int(bad[0])
        return (f"{what}: returned cloud differs at {len(bad)} of {len(g)} records, first at position {k}: "
                f"{g[k].view(synth.POINT_DTYPE)[0]} != {w[k].view(synth.POINT_DTYPE)[0]}")
    for name in LAYERS:
        a, b = canonical_bits(got_layers[name]), canonical_bits(want_layers[name])
        if a.shape != b.shape:
            return f"{what}: layer {name} is {a.shape}, expected {b.shape}"
        d = np.argwhere(a != b)
        if len(d):
            i, j = (int(v) for v in d[0])
            return (f"{what}: layer {name} differs in {len(d)} cells, first at ({i}, {j}): "
                    f"{np.asarray(got_layers[name])[i, j]!r} (0x{a[i, j]:08x}) != {np.asarray(want_layers[name])[i, j]!r} (0x{b[i, j]:08x})")
    return ""
