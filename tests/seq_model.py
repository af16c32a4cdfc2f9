"""Random sequences of API calls held to a per-slot model of the CPU oracle.

Three parts, none of which needs a GPU to import:

  make_sequence(seed, shape)   a seeded list of op records (plain dicts: ints, floats, names, lists) that serialises to JSON.  The
                               generator knows the header's preconditions (include/groundgrid_hip.h) and nothing of the library.
  ContextModel                 applies ops to one oracle.OracleMap per slot plus a few host-side facts (own configuration, scoring and
                               counters, the context's configuration / Eigen convention / label list) and returns, per op, what the
                               library must return.  It follows the header, never gg_context.hip.  `mutant` switches on ONE deliberate
                               bookkeeping slip (MUTANTS): tests/test_sequences_cpu.py shows that the sequences tell each from the truth.
  run_on_device(seg, ops, ..)  issues the same ops through groundgrid_amd.api.  Outputs of device ops stay on the device until the next
                               `checkpoint` op (gg_batch_fence on every caller stream used, then one synchronisation), so that the
                               library's own cross-stream ordering is what makes them right.

A result is a dict name -> array / scalar / bytes; first_diff() compares bit for bit (NaN == NaN, -0.0 != 0.0).

The many-map device calls that read or write map state (NEW_KINDS: gg_import_layers, gg_export_images, gg_export_slopes, gg_split_clouds,
gg_rasterize_clouds, gg_cluster_clouds, gg_clearance_clouds in cloud mode, gg_visibility_clouds) are inserted into that list by a second
generator stream (_Ins), so that make_sequence(seed, shape, device_calls=False) stays the list it was.  A cloud call takes its points and
labels from an earlier filter_batch of the sequence (chained: that batch's device buffers, named by the batch's index) or from seeded
data that belong to no batch (foreign).  The model derives what they return from the slot's OracleMap as it stands and the references
of tests/cloud_refs.py, slopes_ref.py, cluster_ref.py, clearance_ref.py and visibility_ref.py; the driver hands them sentinel-filled
destinations with slack words and padded strides, and compares at the next checkpoint, untouched words included.
The six calls on caller-held planes (PLANE_KINDS: gg_fuse_states, gg_route_planes, gg_match_planes, gg_footprint_planes,
gg_route_headings, gg_track_clusters) read and write no map state, so their arithmetic cannot depend on the calls around them -- but they
run in the frame of the other many-map calls (the shared ring of parameter entries, the context's batch and map events), and what they
read is what an earlier call, often on another stream, wrote into a buffer the caller holds.  A third generator stream inserts them the
same way (make_sequence(.., plane_calls=False) is the list as it was); tests/seq_planes.py holds that generator, their part of the model
(the references fusion_ref, route_ref, match_ref, footprint_ref, headings_ref, tracks_ref on the model's own copy of the chained planes)
and their part of the driver.
Three later calls (LATE_KINDS: gg_box_clusters, gg_score_rollouts, gg_clearance_clouds in plane mode) come from a fourth generator
stream behind the third one's tail (make_sequence(.., late_calls=False) is the list as it was); tests/seq_late.py holds that generator,
their part of the model (box_ref, rollouts_ref, clearance_ref) and their part of the driver.
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib.util
import json
import os

import numpy as np

from groundgrid_amd import kitti
from oracle import oracle
from tests import clearance_ref, cloud_refs, seq_late, seq_planes, slopes_ref

LAYERS = list(oracle.LAYERS)
PER_CALL = [k for k in LAYERS if k not in ("ground", "groundpatch")]
LAZY3 = ("maxGroundHeight", "groundCandidates", "planeDist")
BASE_Z = -1.73
PC2_DTYPE = np.dtype({"names": ["x", "y", "z", "intensity", "ring"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 4, 8, 12, 16],
                      "itemsize": 18})

# ---------------------------------------------------------------------------------------------------------------- shapes
# Sizes follow the launch logic (k4_sweep.hip, gg_context.hip): at most 16 clouds take the pair sweep, 17..256 k_sweep in parts, more than
# 256 clouds of fresh maps k_sweep<FRESH>; halves_min_clouds or more clouds run as two streams under GG_FLAG_CONCURRENT_HALVES.
SHAPES = {
    "latency": dict(length=120.0, res=0.33, n_slots=3, stride=2048, pts=(500, 1900), spread=14.0, steps=20, halves_min=2,
                    classes=["1", "2-16"]),
    "fleet": dict(length=43.0, res=0.33, n_slots=40, stride=512, pts=(120, 480), spread=9.0, steps=74, halves_min=8,
                  classes=["1", "2-16", "17-64"]),
    "server": dict(length=26.0, res=0.33, n_slots=300, stride=256, pts=(40, 240), spread=6.0, steps=16, halves_min=0,
                   classes=["1", "2-16", "17-64", "65-256", ">256"]),
}
SEEDS_PER_SHAPE = 2
CLASS_RANGE = {"1": (1, 1), "2-16": (2, 16), "17-64": (17, 64), "65-256": (65, 256), ">256": (257, 300)}
STREAMS = ["default", "s1", "s2"]          # the legacy default stream (torch's current one outside a stream context), two torch streams
MAP_STREAMS = ["ctx"] + STREAMS            # ... and the context's own stream (NULL): resets, moves, batches and exports take all four

# configurations as edits of the defaults (cfg/GroundGrid.cfg): data, so that the model and the driver build the same structs
CONFIGS = [
    {},
    {"max_ring": 40, "outlier_tolerance": 0.05, "min_outlier_detection_ground_confidence": 0.8},
    {"occupied_cells_decrease_factor": 1.1, "patch_size_change_distance": 0.0, "point_count_cell_variance_threshold": 3},
    {"occupied_cells_decrease_factor": 3.0, "patch_size_change_distance": 1e3, "distance_factor": 0.002},
    {"miminum_point_height_threshold": 0.2, "minimum_point_height_obstacle_threshold": 0.05, "minimum_distance_factor": 0.0008,
     "outlier_tolerance": 0.2, "min_outlier_detection_ground_confidence": 0.3},
    {"ground_patch_detection_minimum_point_count_threshold": 0.05, "min_outlier_detection_ground_confidence": 0.5, "outlier_tolerance": 0.3},
]
# `ring` doubles as the SemanticKITTI label id of the evaluator (scripts/kitti_data_publisher.py:124-130)
RING_IDS = np.array([0, 1, 10, 11, 13, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 5, 63, 70, 72], dtype=np.uint16)
LABEL_LISTS = [[40, 44, 48, 49, 70, 72], [0, 1, 10, 11, 13, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99], [48, 10]]
STAGES = ["detect_patches", "spiral", "patch3", "patch5", "interpolate"]

MUTATING = ["reset_maps", "map_reset", "move_maps", "map_move", "set_position", "set_layer", "filter_batch", "filter_cloud", "filter_async2",
            "filter_layers", "filter_pc2", "filter_pc2_out", "insert_cloud", "stage", "set_config", "set_slot_configs", "set_conventions",
            "set_score_labels", "set_scoring", "reset_scores"]
OBSERVING = ["get_layer", "get_layers", "export_layers", "scores", "point_classes", "slot_config", "get_position", "image_u8", "terrain_image",
             "gridmap_message", "synchronize", "batch_fence", "set_flags", "checkpoint"]
OLD_KINDS = MUTATING + OBSERVING   # (set_flags changes no observable -- every layer reads as the reference's at all times -- so it is not "mutating")
# the many-map device calls that read or write map state: drawn from a generator stream of their own and inserted into the list of the
# kinds above (make_sequence), so that a committed seed keeps every op it had
LAYER_READERS = ["export_images", "export_slopes"]
CLOUD_KINDS = ["split_clouds", "rasterize_clouds", "cluster_clouds", "clearance_clouds", "visibility_clouds"]
NEW_READERS = LAYER_READERS + CLOUD_KINDS
NEW_KINDS = ["import_layers"] + NEW_READERS
MUTATING = MUTATING + ["import_layers"]
OBSERVING = OBSERVING + NEW_READERS
# the six calls on caller-held planes (tests/seq_planes.py): a third generator stream, inserted the same way
PLANE_KINDS = list(seq_planes.PLANE_KINDS)
OBSERVING = OBSERVING + PLANE_KINDS
# ... and three that came later (tests/seq_late.py): gg_box_clusters reads the positions of the maps it names, gg_score_rollouts and
# gg_clearance_clouds in plane mode read no map: map i of theirs is row i of their buffers, as for the plane calls
LATE_KINDS = list(seq_late.LATE_KINDS)
OBSERVING = OBSERVING + LATE_KINDS
KINDS = MUTATING + OBSERVING
GLOBAL_KINDS = {"set_config", "set_conventions", "set_score_labels", "set_flags", "synchronize", "batch_fence", "checkpoint"}
DEVICE_KINDS = {"reset_maps", "move_maps", "filter_batch", "export_layers", "batch_fence"} | set(NEW_KINDS) | set(PLANE_KINDS) | set(LATE_KINDS)   # enqueue and return (on a caller stream)
MUTATING_DEVICE_KINDS = {"reset_maps", "move_maps", "filter_batch", "import_layers"}
PARAM_RING = 4   # (gg_context.hip: the entries of the ring of parameter blocks the many-map calls share)
SLOPE_CHANNELS = ["grad_x", "grad_y", "tangent", "normal_z", "step", "min_confidence"]
RASTER_CHANNELS = ["nonground_count", "nonground_max_height", "nonground_min_height", "ground_count", "ground_max_height", "ground_min_height"]
SENTINEL = 0x7FC12345   # what the driver fills every destination with (a NaN no kernel produces); bytes: 0xA5

PREDICATES = ["fresh", "no-confidence", "lazy-owed", "own-config", "scoring", "partly-live"]


def allowed(pred, kind):
    """Does the header allow an op of `kind` on a slot for which `pred` holds?  (gg_get_point_classes speaks of the slot's last filter
    call; a map that was reset and has met no cloud since has none.)"""
    if kind == "checkpoint":
        return False  # (the harness's own synchronisation, not an entry point)
    return not (kind == "point_classes" and pred in ("fresh", "no-confidence"))


# ---------------------------------------------------------------------------------------------------------------- data from specs

_CLOUDS = {}


def cached_cloud(spec, shape):
    key = (shape, spec["seed"], spec["n"], spec["kind"], spec["cx"], spec["cy"])
    if key not in _CLOUDS:
        _CLOUDS[key] = make_cloud(spec, shape)
    return _CLOUDS[key]


def make_cloud(spec, shape):
    """The cloud an op names: {"seed", "n", "kind", "cx", "cy"}; kinds: scene, empty, outside (no point inside the map), nanz (NaN heights)."""
    sh = SHAPES[shape]
    rng = np.random.default_rng([int(spec["seed"]), 77])
    n = 0 if spec["kind"] == "empty" else int(spec["n"])
    half = 0.5 * sh["length"]
    near = rng.normal(0.0, sh["spread"], (n, 2))
    wide = rng.uniform(-1.1 * half, 1.1 * half, (n, 2))
    xy = np.where(rng.random((n, 1)) < 0.7, near, wide)
    x, y = xy[:, 0], xy[:, 1]
    z = -1.7 + 0.02 * x + 0.2 * np.sin(x / 7.0) * np.cos(y / 9.0) + rng.normal(0.0, 0.02, n)
    z = z + np.where(rng.random(n) < 0.15, rng.uniform(0.3, 2.0, n), 0.0)    # clutter above the terrain
    z = z - np.where(rng.random(n) < 0.06, 1.0, 0.0)                          # returns under the terrain: outliers on a confident map
    if spec["kind"] == "nanz":
        z = np.where(rng.random(n) < 0.05, np.nan, z)
    if spec["kind"] == "outside":
        x = x + 3.0 * sh["length"]
    xyz = np.stack([x + spec["cx"], y + spec["cy"], z], axis=1).astype(np.float32)
    return oracle.make_cloud(xyz, ring=rng.choice(RING_IDS, n), intensity=rng.uniform(0.0, 255.0, n).astype(np.float32))


def make_layer(spec, name, n):
    """The (n, n) plane a set_layer op writes: {"seed", "kind"}; contents no cloud produced (after tests/test_gpu_stages_wire.py
    synthetic_layers): patchy counts, heights on a slope, small and large variances, confidences on both sides of every threshold."""
    rng = np.random.default_rng([int(spec["seed"]), 78])
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    slope = (-1.7 + 0.01 * (ii - n / 2) + 0.2 * np.sin(jj / 9.0)).astype(np.float32)
    pts = rng.integers(0, 30, (n, n)).astype(np.float32) * (rng.random((n, n)) < 0.45)
    if spec["kind"] == "fractional":
        pts = (pts * rng.uniform(0.5, 1.5, (n, n))).astype(np.float32)
    if name in ("points", "pointsRaw", "groundCandidates"):
        return pts.astype(np.float32)
    if name == "groundpatch":
        if spec["kind"] == "confident":  # every cell above groundpatch_detection_minimum_threshold and the outlier test's confidence
            return rng.choice(np.array([0.35, 0.55, 0.9, 1.0], dtype=np.float32), (n, n))
        return rng.choice(np.array([0.0, 1e-7, 0.2, 0.45, 0.55, 0.9, 1.0], dtype=np.float32), (n, n))
    if name == "ground":
        return (slope + rng.normal(0, 0.3, (n, n))).astype(np.float32)
    if name == "minGroundHeight":
        return np.where(pts > 0, slope + rng.normal(0, 0.02, (n, n)), 100.0).astype(np.float32)
    if name == "maxGroundHeight":
        return np.where(pts > 0, slope + 0.3, -100.0).astype(np.float32)
    if name in ("m2", "variance", "meanVariance"):
        return (pts * rng.choice(np.array([1e-5, 3e-4, 2e-2], dtype=np.float32), (n, n)) * rng.random((n, n))).astype(np.float32)
    return rng.normal(0, 0.5, (n, n)).astype(np.float32)  # planeDist


def oracle_config(index):
    c = oracle.default_config()
    for k, v in CONFIGS[index].items():
        setattr(c, k, v)
    return c


def config_tuple(c):
    return tuple(getattr(c, name) for name, _ in oracle.Config._fields_)


def to_pc2(cloud):
    out = np.zeros(cloud.shape[0], dtype=PC2_DTYPE)
    for k in ("x", "y", "z", "intensity", "ring"):
        out[k] = cloud[k]
    return out


def pack_masks(labels):
    """gg_batch.d_label_masks: point p in bits 2 * (p % 4) of byte p / 4: 0 dropped, 1 ground, 2 non-ground"""
    code = np.zeros(256, dtype=np.uint8)
    code[49], code[99] = 1, 2
    c = code[labels]
    c = np.concatenate([c, np.zeros((-len(c)) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


_pin = None


def _gridmap_bytes(*a, **k):
    """the grid_map_msgs/GridMap layout restated on the host: tools/pin/compare.py gridmap_message_bytes"""
    global _pin
    if _pin is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pin", "compare.py")
        spec = importlib.util.spec_from_file_location("pin_compare", path)
        _pin = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_pin)
    return _pin.gridmap_message_bytes(*a, **k)


def image_u8_reference(L):
    """grid_map::GridMapCvConverter::toImage<unsigned char, 1> restated with numpy (tests/test_gpu_parity.py)"""
    fin = np.isfinite(L)
    lo, hi = np.float32(L[fin].min()), np.float32(L[fin].max())
    with np.errstate(all="ignore"):
        e = ((np.clip(L, lo, hi) - lo) / (hi - lo)) * np.float32(255.0)
        img = np.where(fin & np.isfinite(e), e, 0).astype(np.uint8)
    return img, lo, hi


def terrain_reference(ground, raw):
    """the 32FC3 terrain image (src/GroundGridNodelet.cpp:247-268): channel 1 only inside the border and only where the 3x3 sum is
    order-free (integer-valued counts)"""
    out = {"ground": ground.copy(), "raw": raw.copy()}
    if np.all(raw == np.round(raw)) and np.all(np.abs(raw) < 1e5):
        s = np.zeros_like(raw)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                s[1:-1, 1:-1] += raw[1 + di: raw.shape[0] - 1 + di, 1 + dj: raw.shape[1] - 1 + dj]
        out["visited"] = (s[1:-1, 1:-1] >= 27).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------- comparing

def _bits(v):
    if isinstance(v, (bytes, bytearray)):
        return np.frombuffer(bytes(v), dtype=np.uint8)
    a = np.ascontiguousarray(v)
    if a.dtype.names or a.dtype.kind == "V":
        return np.frombuffer(a.tobytes(), dtype=np.uint8)
    if a.dtype == np.float32:
        b = a.view(np.uint32).copy()
        b[np.isnan(a)] = 0x7FC00000  # (NaN == NaN; -0.0 and 0.0 keep their own bits)
        return b
    if a.dtype == np.float64:
        b = a.view(np.uint64).copy()
        b[np.isnan(a)] = 0x7FF8000000000000
        return b
    return a


def first_diff(want, got):
    """None, or a description of the first item of `want` that `got` does not match: key and element index (for a layer: the cell)"""
    if want is None:
        return None
    for key, w in want.items():
        if key not in got:
            return f"{key}: missing"
        g = got[key]
        if isinstance(w, (list, tuple)) and not isinstance(w, np.ndarray) and len(w) and isinstance(w[0], (np.ndarray, bytes)):
            if len(w) != len(g):
                return f"{key}: {len(g)} items, expected {len(w)}"
            for i, (wi, gi) in enumerate(zip(w, g)):
                if isinstance(wi, bytes) and len(gi) > len(wi):
                    gi = bytes(gi[: len(wi)])  # (a returned-cloud row: compared over the length the model expects)
                d = first_diff({f"{key}[{i}]": wi}, {f"{key}[{i}]": gi})
                if d:
                    return d
            continue
        a, b = _bits(np.asarray(w) if not isinstance(w, (bytes, bytearray)) else w), _bits(np.asarray(g) if not isinstance(g, (bytes, bytearray)) else g)
        if a.shape != b.shape:
            return f"{key}: shape {b.shape}, expected {a.shape}"
        if a.dtype != b.dtype:
            return f"{key}: dtype {b.dtype}, expected {a.dtype}"
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            at = tuple(int(v) for v in bad[0])
            wv, gv = np.asarray(w) if not isinstance(w, (bytes, bytearray)) else a, np.asarray(g) if not isinstance(g, (bytes, bytearray)) else b
            try:
                shown = f"got {gv[at]!r}, expected {wv[at]!r}"
            except Exception:
                shown = "bytes differ"
            return f"{key}: {len(bad)} elements differ, first at {list(at)}: {shown}"
    return None


# ---------------------------------------------------------------------------------------------------------------- the generator

def _pair_table():
    """every (predicate or None, op kind) the coverage table asks for, in one fixed shuffled order, dealt to the committed sequences in
    proportion to their step counts"""
    pairs = [(p, k) for p in PREDICATES + [None] for k in OLD_KINDS if allowed(p, k)]
    order = np.random.default_rng(20260101).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    deal = []
    for name, sh in SHAPES.items():
        for s in range(SEEDS_PER_SHAPE):
            deal += [(name, s)] * sh["steps"]
    deal = [deal[i] for i in np.random.default_rng(20260102).permutation(len(deal))]
    out = {}
    for i, pair in enumerate(pairs):
        out.setdefault(deal[i % len(deal)], []).append(pair)
    return out


class _Gen:
    def __init__(self, seed, shape):
        self.shape, self.sh, self.seed = shape, SHAPES[shape], int(seed)
        self.rng = np.random.default_rng([int(seed), list(SHAPES).index(shape)])
        self.n = self.sh["n_slots"]
        self.ops = []
        self.pos = [(0.0, 0.0)] * self.n          # where the generator believes each map lies (to aim clouds; whole cells do not matter)
        self.cloud_n = [None] * self.n            # size of the slot's last filter-call cloud, while gg_get_point_classes may ask for it
        self.labels_set = False
        self.flags = dict(minimal=False, eager=False, halves=False)
        self.cloud_seed = 1000 * (self.seed + 1)
        self.cursor = {}
        self.cells = oracle.OracleMap(self.sh["length"], self.sh["res"]).rows

    # -- pieces
    def emit(self, op, **kw):
        self.ops.append(dict(op=op, **kw))

    def r(self, lo, hi):
        return round(float(self.rng.uniform(lo, hi)), 3)

    def slot(self):
        return int(self.rng.integers(0, self.n))

    def slots(self, count, must=None):
        count = min(count, self.n)
        pick = [int(v) for v in self.rng.permutation(self.n)[:count]]
        if must is not None and must not in pick:
            pick[int(self.rng.integers(0, count))] = must
        return pick

    def cloud(self, slot, kind=None, tf=False):
        self.cloud_seed += 1
        if kind is None:
            u = self.rng.random()
            kind = "empty" if u < 0.03 else "outside" if u < 0.06 else "nanz" if u < 0.16 else "scene"
        lo, hi = self.sh["pts"]
        cx, cy = (0.0, 0.0) if tf else self.pos[slot]
        return dict(seed=self.cloud_seed, n=int(self.rng.integers(lo, hi)), kind=kind, cx=cx, cy=cy)

    def pose(self, slot):
        """map <- sensor: the map's position, a small tilt and a yaw (tx, ty, tz, qx, qy, qz, qw)"""
        th = float(self.rng.uniform(-0.6, 0.6))
        q = np.array([self.r(-0.01, 0.01), self.r(-0.01, 0.01), np.sin(th / 2), np.cos(th / 2)])
        q = q / np.linalg.norm(q)
        return [self.pos[slot][0], self.pos[slot][1], self.r(-0.05, 0.05)] + [float(v) for v in q]

    def single(self, slot, tf=None, kind=None):
        tf = bool(self.rng.random() < 0.4) if tf is None else tf
        pose = self.pose(slot) if tf else None
        org = [self.pos[slot][0] + self.r(-0.3, 0.3), self.pos[slot][1] + self.r(-0.3, 0.3), self.r(-0.05, 0.05)]
        return dict(slot=slot, cloud=self.cloud(slot, kind, tf), origin=org, base_z=BASE_Z + self.r(-0.02, 0.02), tf=pose)

    def base_pose(self):
        """base_link <- map of GroundGrid::update"""
        th = float(self.rng.uniform(-0.3, 0.3))
        q = np.array([self.r(-0.02, 0.02), self.r(-0.02, 0.02), np.sin(th / 2), np.cos(th / 2)])
        q = q / np.linalg.norm(q)
        return [self.r(-1, 1), self.r(-1, 1), self.r(1.4, 1.9)] + [float(v) for v in q]

    def odom(self, slot):
        u = self.rng.random()
        res, length = self.sh["res"], self.sh["length"]
        x, y = self.pos[slot]
        if u < 0.04:
            d = (0.0, 0.0)                                              # no shift
        elif u < 0.12:
            d = (1.5 * length * float(self.rng.choice([-1, 1])), self.r(-2, 2))   # further than the map is long
        else:
            d = (self.r(1.2, 9) * res * float(self.rng.choice([-1, 1])), self.r(0, 9) * res * float(self.rng.choice([-1, 1])))
        self.pos[slot] = (round(x + d[0], 3), round(y + d[1], 3))
        return list(self.pos[slot])

    def next_of(self, names, attr):
        k = self.cursor.get(attr, 0)
        self.cursor[attr] = k + 1
        return names[k % len(names)]

    # -- ops by kind (each names `slot` among the maps it touches where it touches any)
    def op(self, kind, slot):
        g = getattr(self, "op_" + kind)
        g(slot)

    def op_reset_maps(self, slot, stream=None, persistent=None):
        count = int(self.rng.integers(1, max(2, min(self.n, 12 if self.rng.random() < 0.7 else self.n) + 1)))
        first = int(np.clip(slot - int(self.rng.integers(0, count)), 0, self.n - count))
        pos = [self.r(-30, 30), self.r(-30, 30)]
        persistent = bool(self.rng.random() < 0.3) if persistent is None else persistent
        self.emit("reset_maps", first=first, n=count, odom_z=self.r(-1.9, -1.5), pos=pos, persistent=persistent,
                  stream=stream or self.next_of(MAP_STREAMS, "reset stream"))
        for s in range(first, first + count):
            self.pos[s] = tuple(pos)
            if not persistent:
                self.cloud_n[s] = None

    def op_map_reset(self, slot):
        pos = [self.r(-30, 30), self.r(-30, 30)]
        self.emit("map_reset", slot=slot, odom_z=self.r(-1.9, -1.5), pos=pos)
        self.pos[slot], self.cloud_n[slot] = tuple(pos), None

    def op_move_maps(self, slot, stream=None):
        sl = self.slots(int(self.rng.integers(1, min(self.n, 24) + 1)), slot)
        self.emit("move_maps", slots=sl, odoms=[self.odom(s) for s in sl], poses=[self.base_pose() for _ in sl],
                  stream=stream or self.next_of(MAP_STREAMS, "move stream"))

    def op_map_move(self, slot):
        self.emit("map_move", slot=slot, odom=self.odom(slot), pose=self.base_pose())

    def op_set_position(self, slot):
        x, y = self.pos[slot]
        self.pos[slot] = (round(x + self.r(-2, 2), 3), round(y + self.r(-2, 2), 3))
        self.emit("set_position", slot=slot, pos=list(self.pos[slot]))

    def op_set_layer(self, slot, layer=None, kind=None):
        layer = layer or LAYERS[int(self.rng.integers(0, len(LAYERS)))]
        self.cloud_seed += 1
        self.emit("set_layer", slot=slot, layer=layer, fill=dict(seed=self.cloud_seed, kind=kind or str(self.rng.choice(["integer", "fractional", "confident"]))))

    def op_filter_batch(self, slot, stream=None, count=None, outputs=None):
        if count is None:
            lo, hi = CLASS_RANGE[self.next_of(self.sh["classes"], "k_class")]
            count = int(self.rng.integers(lo, min(hi, self.n) + 1))
        sl = self.slots(count, slot)
        fmt, tf = self.next_of([(16, False), (32, True), (32, False), (16, True), (16, False), (32, False)], "batch format")
        items = [self.single(s, tf=tf) for s in sl]
        if outputs is None:
            names = ["labels", "out_index", "counts", "masks", "pc2"] + (["out_clouds"] if fmt == 32 else [])
            outputs = [k for k in names if self.rng.random() < 0.6]
        self.emit("filter_batch", slots=sl, clouds=[i["cloud"] for i in items], origins=[i["origin"] for i in items],
                  base_z=[i["base_z"] for i in items], tfs=[i["tf"] for i in items] if tf else None, fmt=fmt, outputs=outputs,
                  stream=stream or self.next_of(MAP_STREAMS, "batch stream"))
        for s, i in zip(sl, items):
            self.cloud_n[s] = 0 if i["cloud"]["kind"] == "empty" else i["cloud"]["n"]

    def _single(self, kind, slot, **kw):
        i = self.single(slot)
        self.emit(kind, **i, **kw)
        self.cloud_n[slot] = 0 if i["cloud"]["kind"] == "empty" else i["cloud"]["n"]

    def op_filter_cloud(self, slot):
        self._single("filter_cloud", slot)

    def op_filter_async2(self, slot):
        other = slot if self.rng.random() < 0.5 else self.slot()
        items = [self.single(slot), self.single(other)]
        self.emit("filter_async2", items=items)
        for i in items:
            self.cloud_n[i["slot"]] = 0 if i["cloud"]["kind"] == "empty" else i["cloud"]["n"]

    def op_filter_layers(self, slot):
        names = [k for k in LAYERS if self.rng.random() < 0.5] or ["ground"]
        self._single("filter_layers", slot, layers=names, registered=bool(self.rng.random() < 0.5))

    def op_filter_pc2(self, slot):
        self._single("filter_pc2", slot)

    def op_filter_pc2_out(self, slot):
        self._single("filter_pc2_out", slot)

    def op_insert_cloud(self, slot):
        c = self.cloud(slot, kind="scene")
        a, b = sorted(int(v) for v in self.rng.integers(0, c["n"] + 1, 2))
        self.emit("insert_cloud", slot=slot, cloud=c, start=a, end=b, origin=[self.pos[slot][0], self.pos[slot][1], 0.0])
        self.cloud_n[slot] = None

    def op_stage(self, slot, stage=None):
        stage = stage or str(self.rng.choice(STAGES))
        n = self.cells
        self.emit("stage", slot=slot, stage=stage, section=int(self.rng.integers(-1, 4)), i=int(self.rng.integers(2, n - 2)),
                  j=int(self.rng.integers(2, n - 2)), base_z=BASE_Z + self.r(-0.2, 0.2))

    def op_set_config(self, slot, index=None):
        self.emit("set_config", cfg=int(self.rng.integers(0, len(CONFIGS))) if index is None else index)

    def op_set_slot_configs(self, slot, clear=None):
        sl = self.slots(int(self.rng.integers(1, min(self.n, 8) + 1)), slot)
        clear = bool(self.rng.random() < 0.3) if clear is None else clear
        self.emit("set_slot_configs", slots=sl, cfgs=None if clear else [int(self.rng.integers(1, len(CONFIGS))) for _ in sl])

    def op_set_conventions(self, slot):
        self.emit("set_conventions", eigen=int(self.rng.integers(0, 2)))

    def op_set_flags(self, slot, **kw):
        f = dict(minimal=bool(self.rng.random() < 0.5), eager=bool(self.rng.random() < 0.3), halves=bool(self.rng.random() < 0.5))
        f.update(kw)
        self.flags = f
        self.emit("set_flags", **f)

    def op_set_score_labels(self, slot):
        self.emit("set_score_labels", ids=LABEL_LISTS[int(self.rng.integers(0, len(LABEL_LISTS)))])
        self.labels_set = True

    def need_labels(self):
        if not self.labels_set:
            self.op_set_score_labels(0)

    def op_set_scoring(self, slot, enable=None):
        self.need_labels()
        sl = self.slots(int(self.rng.integers(1, min(self.n, 10) + 1)), slot)
        self.emit("set_scoring", slots=sl, enable=bool(self.rng.random() < 0.75) if enable is None else enable)

    def op_reset_scores(self, slot):
        self.need_labels()
        self.emit("reset_scores", slots=self.slots(int(self.rng.integers(1, min(self.n, 6) + 1)), slot))

    def op_get_layer(self, slot, layer=None):
        self.emit("get_layer", slot=slot, layer=layer or LAYERS[int(self.rng.integers(0, len(LAYERS)))])

    def op_get_layers(self, slot):
        self.emit("get_layers", slot=slot, names=None if self.rng.random() < 0.5 else ([k for k in LAYERS if self.rng.random() < 0.4] or ["variance"]))

    def op_export_layers(self, slot, stream=None):
        sl = self.slots(int(self.rng.integers(1, min(self.n, 20) + 1)), slot)
        names = LAYERS if self.rng.random() < 0.4 else ([k for k in LAYERS if self.rng.random() < 0.4] or ["ground", "groundpatch"])
        self.emit("export_layers", slots=sl, names=list(names), row_major=bool(self.rng.random() < 0.5),
                  stream=stream or self.next_of(MAP_STREAMS, "export stream"), pad=self.next_of([0, 37, 0, 1], "export pad"))

    def op_scores(self, slot):
        self.need_labels()
        self.emit("scores", slots=self.slots(int(self.rng.integers(1, min(self.n, 12) + 1)), slot))

    def op_point_classes(self, slot):
        if not self.cloud_n[slot]:  # (the header speaks of the points of the slot's last filter call: give it one that has some)
            self.emit("filter_cloud", **self.single(slot, kind="scene"))
            self.cloud_n[slot] = self.ops[-1]["cloud"]["n"]
        self.emit("point_classes", slot=slot, n=self.cloud_n[slot])

    def op_slot_config(self, slot):
        self.emit("slot_config", slot=slot)

    def op_get_position(self, slot):
        self.emit("get_position", slot=slot)

    def op_image_u8(self, slot):
        self.emit("image_u8", slot=slot, layer=LAYERS[int(self.rng.integers(0, len(LAYERS)))])

    def op_terrain_image(self, slot):
        self.emit("terrain_image", slot=slot)

    def op_gridmap_message(self, slot):
        self.emit("gridmap_message", slot=slot, layers=None if self.rng.random() < 0.5 else ([k for k in LAYERS if self.rng.random() < 0.4] or ["ground"]),
                  seq=int(self.rng.integers(0, 1000)), stamp=[int(self.rng.integers(0, 2 ** 31)), int(self.rng.integers(0, 10 ** 9))])

    def op_synchronize(self, slot):
        self.emit("synchronize")

    def op_batch_fence(self, slot):
        self.emit("batch_fence", stream=self.next_of(STREAMS, "fence stream"))

    def op_checkpoint(self, slot=None):
        self.emit("checkpoint")

    # -- bring a predicate about on `slot` (what the header says brings it about)
    def establish(self, pred, slot):
        if pred == "fresh":
            self.op_reset_maps(slot)
        elif pred == "no-confidence":
            if self.rng.random() < 0.5:
                self.op_map_reset(slot)
            else:
                self.op_reset_maps(slot, persistent=False)
            if self.rng.random() < 0.5:
                self.op_get_layer(slot, "ground")   # (a reader: no longer unwritten, still without a confident cell)
        elif pred == "lazy-owed":
            if self.flags["eager"]:
                self.op_set_flags(slot, eager=False)
            self.op_filter_batch(slot, count=int(self.rng.integers(1, min(self.n, 6) + 1)))
        elif pred == "own-config":
            self.op_set_slot_configs(slot, clear=False)
        elif pred == "scoring":
            self.op_set_scoring(slot, enable=True)
        elif pred == "partly-live":
            self.op_filter_cloud(slot)
            if self.rng.random() < 0.5:
                self.op_get_layer(slot, "variance")
            else:
                self.op_set_layer(slot, layer=str(self.rng.choice(PER_CALL)))

    def burst(self, variant):
        """device ops in a row on two streams with no host synchronisation between them, then a checkpoint; the four bursts of a
        shape's two committed seeds take every pair of caller streams"""
        s = self.slot()
        a, b = [("s1", "s2"), ("s2", "default"), ("default", "s1"), ("s2", "s1")][variant % 4]
        if variant % 2 == 0:
            self.op_filter_batch(s, stream=a)
            self.op_export_layers(s, stream=b)
            self.op_move_maps(s, stream=a)
            self.op_filter_batch(s, stream=b)
            self.op_reset_maps(s, stream=a, persistent=True)
            self.op_move_maps(s, stream=b)
            self.op_filter_batch(s, stream=b)
            self.op_export_layers(s, stream=a)
        else:
            self.op_reset_maps(s, stream=a)
            self.op_filter_batch(s, stream=b)
            self.op_filter_batch(s, stream=a)
            self.op_export_layers(s, stream=b)
            self.op_move_maps(s, stream="ctx")
            self.op_move_maps(s, stream=a)
            self.op_filter_batch(s, stream=b)
            self.op_export_layers(s, stream=a)
            self.op_move_maps(s, stream=b)
        self.op_checkpoint()

    def stale_confidence_script(self):
        """reset -> set("groundpatch", values > 0.01) -> a filter call under a configuration whose outlier test trusts such cells: the one
        place where a stale "this map has no confident cell" would show"""
        s = self.slot()
        self.op_set_config(s, index=5)
        self.op_reset_maps(s, persistent=False)
        self.op_set_layer(s, layer="groundpatch", kind="confident")
        if self.rng.random() < 0.5:
            self.op_filter_batch(s, count=min(self.n, 3))
        else:
            self.emit("filter_cloud", **self.single(s, tf=False, kind="scene"))
            self.cloud_n[s] = self.ops[-1]["cloud"]["n"]
        self.op_get_layers(s)

    def stage_script(self):
        """the stages on layers no cloud produced (fractional counts: the order of the 5x5 sums shows), under the other Eigen convention"""
        s = self.slot()
        self.emit("set_conventions", eigen=1)
        for layer in ("points", "m2", "minGroundHeight", "groundpatch", "ground"):
            self.op_set_layer(s, layer=layer, kind="fractional")
        self.emit("stage", slot=s, stage="detect_patches", section=-1, i=2, j=2, base_z=BASE_Z)
        self.emit("stage", slot=s, stage="spiral", section=-1, i=2, j=2, base_z=BASE_Z)
        self.op_get_layers(s)
        self.op_set_conventions(s)

    def config_script(self):
        """a slot gets its own configuration, gives it back, and has to follow the context's next one"""
        s = self.slot()
        self.emit("set_slot_configs", slots=[s], cfgs=[4])
        self.emit("set_slot_configs", slots=[s], cfgs=None)
        self.op_set_config(s, index=int(self.rng.choice([1, 2, 3])))
        self._single("filter_cloud", s)
        self.op_get_layers(s)
        self.op_slot_config(s)

    def lazy_set_script(self):
        """one of the three lazily kept layers is set while it is still owed, then read"""
        s = self.slot()
        if self.flags["eager"]:
            self.op_set_flags(s, eager=False)
        self.op_filter_batch(s, count=min(self.n, 2))
        self.op_set_layer(s, layer="planeDist")
        self.op_get_layer(s, "planeDist")

    def insert_script(self):
        """insert_cloud on top of what a cloud left, read before the next filter call resets the per-call layers"""
        s = self.slot()
        self._single("filter_cloud", s)
        self.op_insert_cloud(s)
        self.op_get_layer(s, "points")

    def read_back_script(self):
        """every kind of filter call, move and reset once with a reader right behind it, and a scored slot whose counters are zeroed
        between two clouds"""
        s = self.slot()
        self.need_labels()
        self.emit("set_scoring", slots=[s], enable=True)
        for kind in ("filter_cloud", "filter_async2", "filter_layers", "filter_pc2", "filter_pc2_out", "map_move", "move_maps", "set_position",
                     "map_reset"):
            self.op(kind, s)
            self.op_get_layer(s, "ground")
            self.op_get_position(s)
        self.op_filter_batch(s, stream="ctx", count=min(self.n, 3))    # the context's own stream: the hand-over in the other direction
        self.op_export_layers(s, stream="ctx")
        self.op_move_maps(s, stream="s1")
        self.op_filter_batch(s, stream="ctx", count=min(self.n, 2))
        self.op_checkpoint()
        self._single("filter_cloud", s)
        self.emit("reset_scores", slots=[s])
        self._single("filter_pc2_out", s)
        self.emit("scores", slots=[s])

    def fresh_sweep_script(self):
        """every map re-initialised, then more than 256 of them in one batch: the launch that sweeps fresh maps as they are"""
        self.emit("reset_maps", first=0, n=self.n, odom_z=self.r(-1.9, -1.5), pos=[0.0, 0.0], persistent=False, stream=self.next_of(MAP_STREAMS, "reset stream"))
        self.pos = [(0.0, 0.0)] * self.n
        self.cloud_n = [None] * self.n
        self.op_set_flags(0, halves=True)
        for fenced in ((True, False) if self.seed % 2 == 0 else (False, True)):
            self.op_filter_batch(self.slot(), count=int(self.rng.integers(257, self.n + 1)), stream="s1")   # (divided: two streams)
            if fenced:
                self.emit("batch_fence", stream="s1")
            self.op_filter_batch(self.slot(), count=int(self.rng.integers(257, self.n + 1)), stream="s2")
        self.op_checkpoint()

    def run(self):
        sh = self.sh
        self.emit("tunings", graphs=int(self.seed % 2) if self.shape == "latency" else 0, halves_min_clouds=sh["halves_min"],
                  front=int(self.rng.integers(0, 4)), sweep_waves=int(self.rng.choice([0, 0, 2])), scan_parts=int(self.rng.choice([0, 0, 2])),
                  move_chunk=int(self.rng.choice([0, 0, 3])), export_variant=int(self.rng.integers(0, 2)))
        if self.shape != "latency":
            self.op_set_flags(0, halves=True)
        pairs = list(_pair_table().get((self.shape, self.seed % SEEDS_PER_SHAPE), []))
        if self.seed >= SEEDS_PER_SHAPE:  # (a seed beyond the committed ones: the same cells in another order)
            pairs = [pairs[i] for i in self.rng.permutation(len(pairs))]
        steps = max(sh["steps"], len(pairs))
        for step in range(steps):
            if step in (steps // 4, (3 * steps) // 4):
                self.burst(2 * self.seed + int(step > steps // 4))
            if step == 1:   # (early: a wrong model is then told from the right one after few ops)
                self.stale_confidence_script()
                self.stage_script()
                self.config_script()
                self.lazy_set_script()
                self.insert_script()
                self.read_back_script()
                if self.n > 256:
                    self.fresh_sweep_script()
            if step < len(pairs):
                pred, kind = pairs[step]
            else:
                pred, kind = None, OLD_KINDS[int(self.rng.integers(0, len(OLD_KINDS)))]
            if kind == "checkpoint":
                kind = "synchronize"
            slot = self.slot()
            if pred is not None:
                self.establish(pred, slot)
            self.op(kind, slot)
            if step % 5 == 4:
                self.op_checkpoint()
        self.op_checkpoint()
        return self.ops


def _new_pairs(shape, seed):
    """the (predicate or None, new kind) pairs the inserter of (shape, seed) tries to bring about: every kind with no predicate in every
    sequence, every other pair in two of the six committed ones"""
    pairs = [(p, k) for p in PREDICATES for k in NEW_KINDS if allowed(p, k)]
    pairs = [pairs[i] for i in np.random.default_rng(20261019).permutation(len(pairs))]
    q = 2 * list(SHAPES).index(shape) + int(seed) % SEEDS_PER_SHAPE
    total = len(SHAPES) * SEEDS_PER_SHAPE
    return [(None, k) for k in NEW_KINDS] + [pair for t, pair in enumerate(pairs) if q in (t % total, (t + 3) % total)]


class _Ins:
    """Inserts ops of NEW_KINDS into the list `old` of the other kinds, which stays a subsequence with every dict as it was.  A generator
    stream of its own; like _Gen it knows the header's preconditions and nothing of the library.  Four sources of insertions:
      anchors   next to a mutating device op (or an export, for the import) of the old list, on ANOTHER stream and on one of its maps: the
                reader behind it (read after write) or in front of it (write after read); a cloud call behind a batch takes that batch's
                cloud and label buffers (chained)
      pairs     _new_pairs, wherever a slot happens to satisfy the predicate; what is left at the end is brought about there
      ring      once, more than PARAM_RING new ops in a row on two streams
      tail      short scripts in front of the last checkpoint, one per promise of the import and of the readers (MUTANTS)
    An import is not inserted where it would take a predicate from an old op that is the last of its (predicate, kind) cell."""

    GP = {"ground", "groundpatch"}

    def __init__(self, seed, shape, old):
        self.shape, self.sh, self.seed, self.old = shape, SHAPES[shape], int(seed), old
        self.rng = np.random.default_rng([int(seed), list(SHAPES).index(shape), 20261019])
        self.n = self.sh["n_slots"]
        self.out = []
        self.pos = [(0.0, 0.0)] * self.n
        self.alive = []                   # [(index in out, op)]: batches with a label output since the last checkpoint
        self.pred = Predicates(self.n)    # over the list as it grows
        self.cursor = {}
        self.next_seed = 500000 + 1000 * self.seed
        self.labels_set = False
        self.flags = dict(minimal=False, eager=False, halves=False)
        self.pending = _new_pairs(shape, seed)
        # the old list's own coverage: per op the touched slots for which each predicate holds when the op arrives, and the cell counts
        p = Predicates(self.n)
        self.touch, self.held, self.cells = [], [], {}
        for op in old:
            t = touched(op, self.n) if op["op"] in OLD_KINDS else []
            h = {q: {s for s in t if p.state[q][s]} for q in ("fresh", "no-confidence", "lazy-owed")}
            for q, hs in h.items():
                if hs:
                    self.cells[(q, op["op"])] = self.cells.get((q, op["op"]), 0) + 1
            self.touch.append(set(t))
            self.held.append(h)
            p.apply(op)

    # -- pieces
    def r(self, lo, hi):
        return round(float(self.rng.uniform(lo, hi)), 3)

    def seed_of(self):
        self.next_seed += 1
        return self.next_seed

    def next_of(self, names, attr):
        k = self.cursor.get(attr, 0)
        self.cursor[attr] = k + 1
        return names[k % len(names)]

    def other_stream(self, stream):
        while True:
            s = self.next_of(["s1", "s2", "default", "s2", "s1", "ctx", "default"], "stream")
            if s != stream:
                return s

    def slots(self, count, must):
        pick = [int(v) for v in self.rng.permutation(self.n)[: min(count, self.n)]]
        if must not in pick:
            pick[int(self.rng.integers(0, len(pick)))] = must
        return pick

    def push(self, op):
        k = op["op"]
        if k == "reset_maps":
            for s in range(op["first"], op["first"] + op["n"]):
                self.pos[s] = tuple(op["pos"])
        elif k in ("map_reset", "set_position"):
            self.pos[op["slot"]] = tuple(op["pos"])
        elif k == "move_maps":
            for s, o in zip(op["slots"], op["odoms"]):
                self.pos[s] = tuple(o)
        elif k == "map_move":
            self.pos[op["slot"]] = tuple(op["odom"])
        elif k == "set_score_labels":
            self.labels_set = True
        elif k == "set_flags":
            self.flags = dict(minimal=op["minimal"], eager=op["eager"], halves=op["halves"])
        elif k == "checkpoint":
            self.alive = []
        elif k == "filter_batch" and ("labels" in op["outputs"] or "masks" in op["outputs"]):
            self.alive.append((len(self.out), op))
        self.out.append(op)
        self.pred.apply(op)
        if k in NEW_KINDS:   # a pair that this op happens to meet is no longer looked for
            sl = touched(op, self.n)
            self.pending = [(p, kk) for p, kk in self.pending if not (kk == k and (p is None or self._held_before(p, sl)))]

    def _held_before(self, p, slots):
        return any(self._before[p][s] for s in slots)

    def emit(self, op):
        self._before = {p: list(v) for p, v in self.pred.state.items()} if op["op"] in NEW_KINDS else None
        self.push(op)

    # -- the import's safety rule
    def import_ok(self, j, slots, names):
        ends = (["fresh", "no-confidence"] if set(names) & self.GP else []) + (["lazy-owed"] if set(names) & set(PER_CALL) else [])
        gone, lost = [], {}
        for s in slots:
            for p in ends:
                for i in range(j, len(self.old)):
                    if s not in self.touch[i]:
                        continue
                    if s not in self.held[i][p]:
                        break
                    gone.append((i, p, s))
        left = {}
        for i, p, s in gone:
            left.setdefault((i, p), set(self.held[i][p])).discard(s)
        for (i, p), rest in left.items():
            if not rest:
                cell = (p, self.old[i]["op"])
                lost[cell] = lost.get(cell, 0) + 1
        if any(self.cells[cell] - k < 1 for cell, k in lost.items()):
            return False
        for (i, p), rest in left.items():
            self.held[i][p] = rest
        for cell, k in lost.items():
            self.cells[cell] -= k
        return True

    # -- the new ops
    def layer_names(self, must_gp=None):
        names = [k for k in LAYERS if self.rng.random() < 0.3]
        if must_gp is True and not set(names) & self.GP:
            names.append(str(self.rng.choice(["ground", "groundpatch"])))
        return [k for k in LAYERS if k in names] or ["ground"]

    def mk_import_layers(self, slot, stream, j, names=None, slots=None, fill=None):
        names = names or self.layer_names()
        slots = slots or self.slots(int(self.rng.integers(1, 4)), slot)
        if j is not None and not self.import_ok(j, slots, names):
            slots = [slot]
            if not self.import_ok(j, slots, names):
                return None
        return dict(op="import_layers", slots=slots, names=names, row_major=bool(self.rng.random() < 0.5), pad=self.next_of([0, 5, 0, 64], "import pad"),
                    fills=[dict(seed=self.seed_of(), kind=fill or str(self.rng.choice(["integer", "fractional", "confident"]))) for _ in slots], stream=stream)

    def mk_export_images(self, slot, stream, names=None, terrain=None):
        names = [k for k in LAYERS if self.rng.random() < 0.25] if names is None else names
        terrain = bool(self.rng.random() < 0.5 or not names) if terrain is None else terrain
        return dict(op="export_images", slots=self.slots(int(self.rng.integers(1, 4)), slot), names=names, terrain=terrain, chw=bool(self.rng.random() < 0.5),
                    pad=self.next_of([0, 3, 0, 32], "image pad"), bounds=bool(self.rng.random() < 0.8), stream=stream)

    def mk_export_slopes(self, slot, stream):
        return dict(op="export_slopes", slots=self.slots(int(self.rng.integers(1, 4)), slot),
                    channels=[k for k in SLOPE_CHANNELS if self.rng.random() < 0.5] or ["step"], row_major=bool(self.rng.random() < 0.5),
                    pad=self.next_of([0, 1, 0, 33], "slopes pad"), stream=stream)

    def source(self, slot, batch=None, foreign=None, cloud_kind=None):
        """(slots, source, masks): chained to an alive batch that holds `slot` (to `batch` = (index, op) where given), else foreign"""
        have = [b for b in self.alive if slot in b[1]["slots"]]
        if batch is None and have and foreign is not True and (foreign is False or self.rng.random() < 0.7):
            batch = have[-1]
        if batch is not None:
            at, bop = batch
            row, B = bop["slots"].index(slot), len(bop["slots"])
            cnt = int(self.rng.integers(1, min(3, B) + 1))
            row0 = int(np.clip(row - int(self.rng.integers(0, cnt)), 0, B - cnt))
            both = "labels" in bop["outputs"] and "masks" in bop["outputs"]
            masks = bool(self.rng.random() < 0.5) if both else "masks" in bop["outputs"]
            return bop["slots"][row0: row0 + cnt], dict(mode="chained", batch=at, row0=row0), masks
        slots = self.slots(int(self.rng.integers(1, 4)), slot)
        tf = bool(self.rng.random() < 0.4)
        masks = bool(self.rng.random() < 0.5)
        clouds, tfs = [], []
        for s in slots:
            u = self.rng.random()
            ck = cloud_kind or ("empty" if u < 0.05 else "outside" if u < 0.2 else "nanz" if u < 0.3 and not tf else "scene")
            cx, cy = (0.0, 0.0) if tf else self.pos[s]
            clouds.append(dict(seed=self.seed_of(), n=int(self.rng.integers(20, min(300, self.sh["stride"]))), kind=ck, cx=cx, cy=cy))
            th = float(self.rng.uniform(-0.6, 0.6))
            q = np.array([self.r(-0.01, 0.01), self.r(-0.01, 0.01), np.sin(th / 2), np.cos(th / 2)])
            tfs.append([self.pos[s][0], self.pos[s][1], self.r(-0.05, 0.05)] + [float(v) for v in q / np.linalg.norm(q)])
        longest = max(c["n"] for c in clouds)
        stride = min(self.sh["stride"], longest + int(self.rng.choice([0, 1, 7, 30])))
        if masks:
            stride = min(self.sh["stride"], 4 * ((stride + 3) // 4))
        return slots, dict(mode="foreign", clouds=clouds, labels=dict(seed=self.seed_of()), fmt=int(self.rng.choice([16, 32])), tfs=tfs if tf else None,
                           stride=stride), masks

    def mk_cloud(self, kind, slot, stream, **src):
        slots, source, masks = self.source(slot, **src)
        op = dict(op=kind, slots=slots, source=source, masks=masks, stream=stream)
        pad = self.next_of([0, 2, 0, 40], "cloud pad")
        band = dict(min_points=int(self.rng.choice([1, 1, 2])), min_height=None if self.rng.random() < 0.5 else self.r(-0.3, 0.2),
                    max_height=None if self.rng.random() < 0.5 else self.r(0.4, 2.5))
        if kind == "split_clouds":
            fields = ["points", "height", "source"]
            want = {s: ([f for f in fields if self.rng.random() < 0.8] or ["height"]) for s in ("ground", "nonground") if self.rng.random() < 0.85}
            op.update(want=want or {"nonground": fields})
        elif kind == "rasterize_clouds":
            op.update(channels=[k for k in RASTER_CHANNELS if self.rng.random() < 0.5] or ["nonground_count"], row_major=bool(self.rng.random() < 0.5), pad=pad)
        elif kind == "cluster_clouds":
            op.update(band, connectivity=int(self.rng.choice([4, 8])), row_major=bool(self.rng.random() < 0.5), pad=pad,
                      max_clusters=int(self.rng.choice([0, 3, 64])), point_clusters=bool(self.rng.random() < 0.7))
        elif kind == "clearance_clouds":
            op.update(band, max_cells=int(self.rng.choice([0, 0, 5, 20])), row_major=bool(self.rng.random() < 0.5), pad=pad,
                      nearest=bool(self.rng.random() < 0.7) and self.shape != "latency", distance=bool(self.rng.random() < 0.7))
        elif kind == "visibility_clouds":
            org = [[self.pos[s][0] + self.r(-0.5, 0.5), self.pos[s][1] + self.r(-0.5, 0.5), self.r(-0.05, 0.05)] for s in slots]
            if self.rng.random() < 0.15:
                org[0][0] += 3.0 * self.sh["length"]   # (a sensor outside its map casts no ray)
            op.update(band, max_cells=int(self.rng.choice([0, 0, 7, 40])), row_major=bool(self.rng.random() < 0.5), pad=pad, origins=org,
                      counts=bool(self.rng.random() < 0.7))
        return op

    def mk(self, kind, slot, stream, j=None, **kw):
        if kind == "import_layers":
            return self.mk_import_layers(slot, stream, j, **kw)
        if kind == "export_images":
            return self.mk_export_images(slot, stream, **kw)
        if kind == "export_slopes":
            return self.mk_export_slopes(slot, stream)
        return self.mk_cloud(kind, slot, stream, **kw)

    def put(self, kind, slot, stream, j=None, **kw):
        op = self.mk(kind, slot, stream, j, **kw)
        if op is not None:
            self.emit(op)
        return op is not None

    # -- where
    @staticmethod
    def guarded(op):
        """tests/test_sequences_cpu.py looks at what stands right behind a batch of more than 256 clouds: nothing goes there"""
        return op["op"] == "batch_fence" or (op["op"] == "filter_batch" and len(op["slots"]) > 256) or op["op"] == "tunings"

    def anchors(self, j):
        """the old op in front of this place and the one behind it"""
        prev, nxt = self.old[j - 1], self.old[j]
        for anchor, after in ((prev, True), (nxt, False)):
            k = anchor["op"]
            if k not in ("filter_batch", "move_maps", "reset_maps", "export_layers") or self.rng.random() >= (0.55 if k == "export_layers" else 0.3):
                continue
            kind = "import_layers" if k == "export_layers" else self.next_of(NEW_READERS + ["import_layers"] + NEW_READERS, "after" if after else "before")
            t = touched(anchor, self.n)
            slot = t[int(self.rng.integers(0, len(t)))]
            kw = {}
            if kind in CLOUD_KINDS and after and k == "filter_batch" and self.alive and self.alive[-1][1] is anchor:
                kw = dict(batch=self.alive[-1])   # (the labels this batch is still writing, read from another stream)
            self.put(kind, slot, self.other_stream(anchor["stream"]), j, **kw)

    def pairs(self, j):
        done = 0
        for pred, kind in list(self.pending):
            if done == 2:
                break
            if pred is None:
                if self.rng.random() >= 0.05:
                    continue
                ok = list(range(self.n))
            else:
                ok = [s for s in range(self.n) if self.pred.state[pred][s]]
            if ok:
                done += self.put(kind, ok[int(self.rng.integers(0, len(ok)))], self.next_of(MAP_STREAMS, "pair stream"), j)

    def ring(self):
        """seven new ops of five kinds in a row on two caller streams: every entry of the shared ring is taken again by another kind"""
        s = self.alive[-1][1]["slots"][0] if self.alive else int(self.rng.integers(0, self.n))
        a, b = [("s1", "s2"), ("default", "s2")][self.seed % 2]
        for kind, st in (("split_clouds", a), ("export_slopes", b), ("rasterize_clouds", a), ("export_images", b), ("cluster_clouds", b),
                         ("visibility_clouds", a), ("clearance_clouds", b)):
            self.put(kind, s, st)

    # -- the tail: old kinds as scaffolding, then the call the script is about
    def establish(self, pred, s):
        if pred in ("fresh", "no-confidence"):
            self.push(dict(op="reset_maps", first=s, n=1, odom_z=self.r(-1.9, -1.5), pos=[self.r(-30, 30), self.r(-30, 30)], persistent=False, stream="s1"))
        elif pred == "lazy-owed":
            self.batch(s, "s2")
        elif pred == "own-config":
            self.push(dict(op="set_slot_configs", slots=[s], cfgs=[int(self.rng.integers(1, len(CONFIGS)))]))
        elif pred == "scoring":
            if not self.labels_set:
                self.push(dict(op="set_score_labels", ids=LABEL_LISTS[0]))
            self.push(dict(op="set_scoring", slots=[s], enable=True))
        elif pred == "partly-live":
            self.push(dict(op="set_layer", slot=s, layer="points", fill=dict(seed=self.seed_of(), kind="integer")))

    def batch(self, s, stream, count=2):
        if self.flags["eager"]:
            self.push(dict(op="set_flags", **dict(self.flags, eager=False)))
        sl = self.slots(count, s)
        lo, hi = self.sh["pts"]
        clouds = [dict(seed=self.seed_of(), n=int(self.rng.integers(lo, hi)), kind="scene", cx=self.pos[t][0], cy=self.pos[t][1]) for t in sl]
        self.push(dict(op="filter_batch", slots=sl, clouds=clouds, origins=[[self.pos[t][0], self.pos[t][1], 0.0] for t in sl], base_z=[BASE_Z for _ in sl],
                       tfs=None, fmt=16, outputs=["labels", "counts", "masks"], stream=stream))

    def tail(self):
        for pred, kind in list(self.pending):
            s = int(self.rng.integers(0, self.n))
            if pred is not None:
                self.establish(pred, s)
            self.put(kind, s, self.next_of(MAP_STREAMS, "pair stream"))
        s = int(self.rng.integers(0, self.n))
        # a fresh map becomes real by the import alone, and its confidence counts for the next cloud's outlier walk
        self.push(dict(op="set_slot_configs", slots=[s], cfgs=None))
        self.push(dict(op="set_config", cfg=5))
        self.establish("fresh", s)
        self.put("import_layers", s, "s2", names=["ground", "groundpatch"], slots=[s], fill="confident")
        self.put("export_slopes", s, "s1")
        self.batch(s, "default")
        self.push(dict(op="get_layers", slot=s, names=None))
        # the three lazily kept layers are computed before an import makes the nine dense, and before their images are taken
        self.batch(s, "s1")
        self.put("import_layers", s, "s2", names=["m2"], slots=[s])
        self.push(dict(op="get_layers", slot=s, names=list(LAZY3)))
        self.batch(s, "s2")
        self.put("export_images", s, "s1", names=["groundCandidates", "planeDist"], terrain=False)
        # a cloud call sees the map where the last move left it, position and terrain
        th = 0.2
        self.push(dict(op="move_maps", slots=[s], odoms=[[round(self.pos[s][0] + 5 * self.sh["res"], 3), round(self.pos[s][1] - 3 * self.sh["res"], 3)]],
                       poses=[[0.3, 0.2, 1.5, 0.0, 0.0, float(np.sin(th / 2)), float(np.cos(th / 2))]], stream="s1"))
        self.put("split_clouds", s, "s2", foreign=False)
        self.put("rasterize_clouds", s, "default", foreign=True, cloud_kind="scene")
        self.push(dict(op="set_position", slot=s, pos=[round(self.pos[s][0] + 1.0, 3), round(self.pos[s][1] + 0.7, 3)]))
        self.put("cluster_clouds", s, "s1", foreign=True, cloud_kind="scene")
        # a fresh map reads as the constant odom_z, whatever lay there before
        self.push(dict(op="reset_maps", first=s, n=1, odom_z=self.r(-1.9, -1.5), pos=list(self.pos[s]), persistent=bool(self.seed % 2), stream="s2"))
        self.put("split_clouds", s, "s1", foreign=True, cloud_kind="scene")
        self.put("export_images", s, "default", names=["ground"], terrain=True)
        self.put("visibility_clouds", s, "s2", foreign=True, cloud_kind="scene")
        # labels that belong to no batch select points outside the map
        self.put("split_clouds", s, "s1", foreign=True, cloud_kind="outside")

    def run(self):
        n = len(self.old)
        ring_at = None
        for j, op in enumerate(self.old):
            if j == n - 1:
                self.tail()
            elif j >= 2 and not self.guarded(self.old[j - 1]) and not self.guarded(op):
                self.anchors(j)
                self.pairs(j)
                if ring_at is None and j > n // 3 and self.old[j - 1]["op"] == "filter_batch" and self.alive:
                    ring_at = j
                    self.ring()
            self.push(op)
        return self.out


def make_sequence(seed, shape, device_calls=True, plane_calls=True, late_calls=True):
    """The op list of (seed, shape): deterministic, JSON-serialisable.  The first record ("tunings") fixes the launch tunings of the
    context for the whole sequence.  device_calls=False: without the ops of NEW_KINDS (and the few ops of other kinds that the last
    scripts put in front of theirs) -- the list as it was before those calls were added, and a subsequence of the full one.
    plane_calls=False: without what the third generator stream adds (every op that carries "g3": the ops of PLANE_KINDS, the cloud calls
    their chains read and the scaffolding of their last scripts) -- the list as it was before the plane calls were added.  A chained
    cloud call of the second stream names its batch by the index in THAT list (mid_indices).
    late_calls=False: without what the fourth generator stream adds behind the third's tail (every op that carries "g4": the ops of
    LATE_KINDS and what their chains need) -- the list as it was before those calls were added.  Its ops stand behind every op of the
    third stream, so no index that one's ops name moves; they carry "g3" too, which goes on counting the ops inserted behind the second
    stream's list."""
    old = _Gen(seed, shape).run()
    if not device_calls:
        return old
    mid = _Ins(seed, shape, old).run()
    return seq_planes.PlaneGen(_this_module(), seed, shape, mid).run(late_calls) if plane_calls else mid


def _this_module():
    import sys

    return sys.modules[__name__]


def mid_indices(ops):
    """the index in `ops` of every op of the list without the third generator stream's, in order"""
    return [i for i, op in enumerate(ops) if "g3" not in op]


def touched(op, n_slots):
    """the slots an op names (every slot for an op that names none)"""
    k = op["op"]
    if k == "reset_maps":
        return list(range(op["first"], op["first"] + op["n"]))
    if k in PLANE_KINDS or k in seq_late.ROW_KINDS:   # (map i of a plane call is row i of its buffers: the call's frame is filled from slots 0 .. n - 1)
        return list(range(min(op["n"], n_slots) if n_slots else op["n"]))
    if k == "box_clusters":   # (a refused call names a slot beyond the context)
        return [s for s in op["slots"] if not n_slots or s < n_slots]
    if k == "filter_async2":
        return [i["slot"] for i in op["items"]]
    if "slots" in op:
        return list(op["slots"])
    if "slot" in op:
        return [op["slot"]]
    return list(range(n_slots))


FILTERS = {"filter_batch", "filter_cloud", "filter_async2", "filter_layers", "filter_pc2", "filter_pc2_out"}


class Predicates:
    """The per-slot predicates of the coverage table, from the op history alone (the header's words, not the library's state):
      fresh          re-initialised by reset_maps / reset; since then only ops named that the header says leave a fresh map as it is
                     (export_layers, scores, a move_maps to where the map already is) or that touch no layer (positions, configurations,
                     scoring switches); a fresh map that scrolls is written, so a move anywhere else ends it
      no-confidence  re-initialised, and no writer of the (ground, confidence) layer since: no filter call, no stage, no set of the two
      lazy-owed      the last cloud came through a call that keeps three layers lazily (filter_batch unless eager; a host call under
                     minimal_layers), and none of the three has been read or set since, nor the map fully re-initialised
      own-config     set_slot_configs gave it a configuration and has not taken it back
      scoring        set_scoring switched it on
      partly-live    since its last cloud a per-call layer was set, or read whole"""

    KEEP_FRESH = {"export_layers", "scores", "set_position", "get_position", "slot_config", "set_slot_configs", "set_scoring", "reset_scores"} | set(NEW_READERS) | set(PLANE_KINDS) | set(seq_late.LATE_KINDS)

    def __init__(self, n_slots):
        self.n = n_slots
        self.state = {p: [False] * n_slots for p in PREDICATES}
        self.flags = dict(minimal=False, eager=False)
        self.where = [(0.0, 0.0)] * n_slots   # the position last given for the map (reset, set_position, a move's odometry)

    def holds(self, pred, slots):
        return any(self.state[pred][s] for s in slots)

    def apply(self, op):
        k, st = op["op"], self.state
        if k == "set_flags":
            self.flags = dict(minimal=op["minimal"], eager=op["eager"])
            return
        if k in GLOBAL_KINDS or k == "tunings":
            return
        reads3 = (k in ("get_layer", "image_u8", "set_layer") and op["layer"] in LAZY3) or \
                 (k in ("get_layers",) and (op["names"] is None or set(op["names"]) & set(LAZY3))) or \
                 (k in ("export_layers", "export_images") and set(op["names"]) & set(LAZY3)) or \
                 (k == "gridmap_message" and (op["layers"] is None or set(op["layers"]) & set(LAZY3))) or \
                 (k == "filter_layers")
        for i, s in enumerate(touched(op, self.n)):
            if k in ("move_maps", "map_move"):
                odom = tuple(op["odoms"][i]) if k == "move_maps" else tuple(op["odom"])
                if k == "map_move" or odom != self.where[s]:
                    st["fresh"][s] = False
                self.where[s] = odom
                continue
            if k in ("reset_maps", "map_reset", "set_position"):
                self.where[s] = tuple(op["pos"])
            if k in ("reset_maps", "map_reset"):
                st["fresh"][s] = st["no-confidence"][s] = True
                if not op.get("persistent", False):
                    st["lazy-owed"][s] = st["partly-live"][s] = False
                continue
            if k == "import_layers":   # (the header's import paragraph: what gg_set_layer of every named layer would leave)
                if set(op["names"]) & {"ground", "groundpatch"}:
                    st["fresh"][s] = st["no-confidence"][s] = False
                if set(op["names"]) & set(PER_CALL):
                    st["lazy-owed"][s], st["partly-live"][s] = False, True
                continue
            if k not in self.KEEP_FRESH:
                st["fresh"][s] = False
            if k in FILTERS or k == "stage" or (k == "set_layer" and op["layer"] in ("ground", "groundpatch")):
                st["no-confidence"][s] = False
            if k in FILTERS:
                lazy = (k == "filter_batch" and not self.flags["eager"]) or (k != "filter_batch" and self.flags["minimal"])
                st["lazy-owed"][s] = lazy and k != "filter_layers"
                st["partly-live"][s] = False
            elif reads3:
                st["lazy-owed"][s] = False
            if (k == "set_layer" and op["layer"] in PER_CALL) or (k == "get_layer" and op["layer"] in PER_CALL) or \
                    (k == "get_layers" and (op["names"] is None or set(op["names"]) & set(PER_CALL))):
                st["partly-live"][s] = True
            if k == "set_slot_configs":
                st["own-config"][s] = op["cfgs"] is not None
            if k == "set_scoring":
                st["scoring"][s] = bool(op["enable"])


# ---------------------------------------------------------------------------------------------------------------- the model

MUTANTS = [
    "fresh_reset_ignored_before_small_batch",   # a map re-initialised by reset_maps keeps its old terrain when a batch of <= 16 clouds meets it next
    "persistent_only_as_full_reset",
    "full_reset_as_persistent_only",
    "own_config_lost_by_reset_maps",
    "own_config_lost_by_move_maps",
    "own_config_lost_by_set_config",
    "cleared_slot_keeps_old_context_config",    # a slot whose own configuration was taken back does not follow a later setConfig
    "lazy_layers_stale_after_set_layer",        # ... a set of one of them is overwritten by the last cloud's values
    "lazy_layers_stale_after_persistent_reset",  # ... they read as before the last cloud
    "move_slots_as_first_plus_i",
    "export_slots_as_first_plus_i",
    "batch_slots_as_first_plus_i",
    "outlier_walk_skipped_after_set_groundpatch",
    "counters_zeroed_by_reset",
    "counters_zeroed_by_move",
    "nonscoring_slot_feeds_counters",
    "eigen_convention_not_applied_to_stage",
    "position_not_updated_for_next_batch",
    # -- the many-map calls (one slip per promise of their header paragraphs)
    "import_leaves_fresh_map_fresh",            # ground / groundpatch imported into a fresh map: it goes on reading as the reset's constants
    "import_groundpatch_keeps_no_confidence",   # ... the next cloud still skips the outlier walk
    "import_drops_lazy_layers",                 # an import of a per-call layer marks all nine dense without computing the three owed ones first
    "import_slots_as_first_plus_i",
    "cloud_reader_position_before_last_move",   # a cloud call computes cells under the position from before the last set_position / move
    "cloud_reader_ground_before_last_scroll",   # ... reads `ground` as it stood before the last move scrolled it
    "fresh_map_read_as_before_reset",           # a reader of a fresh map gets the terrain from before the reset, not the constant odom_z
    "images_read_lazy_layer_uncomputed",        # export_images of one of the three lazily kept layers while it is owed: the stale plane
    "foreign_point_outside_gets_finite_height",  # a selected point outside the map (labels that belong to no batch): 0.0 instead of the quiet NaN
    # -- the calls on caller-held planes (tests/seq_planes.py)
] + list(seq_planes.PLANE_MUTANTS) + list(seq_late.LATE_MUTANTS)   # (... and the three later calls, tests/seq_late.py)
LAZY_MUTANTS = {"import_drops_lazy_layers", "images_read_lazy_layer_uncomputed"}   # (they need what the three layers held before the cloud)


class _Slot:
    def __init__(self, ref):
        self.ref = ref
        self.own = None           # index into CONFIGS, or None: follows the context
        self.frozen = None        # (mutant) the context configuration it stopped following
        self.scoring = False
        self.clouds = 0
        self.counts = np.zeros((65, 2), dtype=np.uint64)
        self.last = None          # (cls, cell) of its last filter call
        self.lazy = False         # (mutants) the three layers are owed; prev3 = what they held before that cloud
        self.prev3 = None
        self.stale_gp = None      # (mutant) (ground, groundpatch) from before a reset the library "forgot"
        self.unconfident = False  # (mutant) the library believes no cell is confident
        self.stale_pos = None     # (mutant) the position from before move_maps
        self.prev_pos = None      # (mutant) the position from before the last set_position / move
        self.prev_ground = None   # (mutant) `ground` from before the last move's scroll, while nothing has written the layer since
        self.stale_ground = None  # (mutant) `ground` from before the last reset_maps


class ContextModel:
    def __init__(self, shape, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.shape, self.sh, self.mutant = shape, SHAPES[shape], mutant
        self.n = self.sh["n_slots"]
        self.slots = [_Slot(oracle.OracleMap(self.sh["length"], self.sh["res"])) for _ in range(self.n)]
        self.rows = self.slots[0].ref.rows
        self.cfg = 0
        self.eigen = 0
        self.ids = None
        self.flags = dict(minimal=False, eager=False, halves=False)
        self._clouds = {}
        self.pred = Predicates(self.n)   # (mutants: which slots are fresh as the header has it)
        self.batches = {}                # op index of a filter_batch -> per row (map-frame cloud, label bytes), until the next checkpoint
        self.at = -1                     # index of the op being applied
        self.outs = {}                   # op index -> {output name: the logical planes per map} of the ops whose planes a plane call may read
        self.shift_log = []              # (op index, slot, shift) of every move: a chain's shifts are sums over it
        self.mid = None                  # bind(): the full index of every op that is not of the third generator stream
        self.mid_seen = []

    # -- helpers
    def cloud(self, spec):
        return cached_cloud(spec, self.shape)

    def config_of(self, s):
        sl = self.slots[s]
        if sl.own is not None:
            return oracle_config(sl.own)
        if sl.frozen is not None:
            return oracle_config(sl.frozen)
        return oracle_config(self.cfg)

    def map_cloud(self, item):
        c = self.cloud(item["cloud"])
        if item.get("tf") is None:
            return c
        M = oracle.matrix_from_pose(item["tf"], "kdl")
        with np.errstate(invalid="ignore", over="ignore"):
            return kitti.transform_cloud(c, M[:, :3], M[:, 3])

    def _filter(self, s, cloud, origin, base_z, lazy, scoring_launch=False):
        sl = self.slots[s]
        m = self.mutant
        if m and (m.startswith("lazy_layers_stale") or m in LAZY_MUTANTS):
            sl.prev3 = {k: sl.ref.layer(k).copy() for k in LAZY3} if lazy else None
        sl.lazy = lazy
        cfg = self.config_of(s)
        if m in ("outlier_walk_skipped_after_set_groundpatch", "import_groundpatch_keeps_no_confidence") and sl.unconfident:
            cfg.min_outlier_detection_ground_confidence = 1e30
        sl.unconfident = False
        sl.prev_ground = None
        pos = None
        if sl.stale_pos is not None:
            pos = tuple(sl.ref._m.contents.position)
            sl.ref._m.contents.position[0], sl.ref._m.contents.position[1] = sl.stale_pos
            sl.stale_pos = None
        sl.ref.cfg = cfg
        oracle.set_eigen_reduction(self.eigen)
        try:
            r = sl.ref.filter_cloud(cloud, tuple(float(np.float32(v)) for v in origin), float(base_z))
        finally:
            oracle.set_eigen_reduction(0)
        if pos is not None:
            sl.ref._m.contents.position[0], sl.ref._m.contents.position[1] = pos
        sl.last = (r["cls"], r["cell"])
        if self.ids is not None and (sl.scoring or (m == "nonscoring_slot_feeds_counters" and scoring_launch)):
            out = r["out_points"]
            keep = ~np.isnan(out["z"])
            bins = np.full(65536, len(self.ids), dtype=np.int64)
            bins[np.asarray(self.ids, dtype=np.int64)] = np.arange(len(self.ids))
            b = bins[out["ring"][keep]]
            g = (out["intensity"][keep] == np.float32(49.0)).astype(np.int64)
            np.add.at(sl.counts, (b, g), 1)
            sl.clouds += 1
        return r

    def _single(self, op, lazy=None):
        lazy = self.flags["minimal"] if lazy is None else lazy
        return self._filter(op["slot"], self.map_cloud(op), op["origin"], op["base_z"], lazy)

    def _touch(self, s):
        """(mutants) an op that is not a small batch looks at the map: the library fills a fresh map then"""
        self.slots[s].stale_gp = None

    def _reset(self, s, pos, odom_z, persistent):
        sl, m = self.slots[s], self.mutant
        if m == "persistent_only_as_full_reset":
            persistent = False
        elif m == "full_reset_as_persistent_only":
            persistent = True
        if m == "lazy_layers_stale_after_persistent_reset" and persistent and sl.lazy and sl.prev3:
            for k in LAZY3:
                sl.ref.set_layer(k, sl.prev3[k])
            sl.lazy = False
        if persistent:
            shape = (self.rows, self.rows)
            sl.ref.set_layer("ground", np.full(shape, np.float32(odom_z)))
            sl.ref.set_layer("groundpatch", np.full(shape, np.float32(0.0000001)))
            sl.ref._m.contents.position[0], sl.ref._m.contents.position[1] = float(pos[0]), float(pos[1])
        else:
            sl.ref.reset_state(pos=(float(pos[0]), float(pos[1])), odom_z=float(np.float32(odom_z)))
            sl.last, sl.lazy = None, False
        sl.unconfident = True
        sl.prev_pos = sl.prev_ground = None
        if m == "counters_zeroed_by_reset":
            sl.counts[...] = 0
            sl.clouds = 0

    def _move(self, s, odom, pose):
        """GroundGrid::update as gg_move_map(s) has it: the two persistent layers scroll; the nine per-call layers stay where they are
        until the next cloud rewrites them (include/groundgrid_hip.h, gg_move_map)"""
        sl, m = self.slots[s], self.mutant
        keep = {k: sl.ref.layer(k).copy() for k in PER_CALL}
        before = tuple(sl.ref._m.contents.position)
        if m == "cloud_reader_ground_before_last_scroll":
            sl.prev_ground = sl.ref.layer("ground").copy()
        moved, shift = sl.ref.update(float(odom[0]), float(odom[1]), pose, "kdl")
        self.shift_log.append((self.at, s, (int(shift[0]), int(shift[1]))))
        if shift == (0, 0):
            sl.prev_ground = None
        sl.prev_pos = before
        for k in PER_CALL:
            sl.ref.set_layer(k, keep[k])
        if m == "counters_zeroed_by_move" and shift != (0, 0):
            sl.counts[...] = 0
            sl.clouds = 0
        return shift, before

    def position(self, s):
        return np.array(tuple(self.slots[s].ref._m.contents.position), dtype=np.float64)

    def state(self, s):
        """everything compared per slot at the end of a sequence"""
        sl = self.slots[s]
        out = {f"layer {k}": sl.ref.layer(k).copy() for k in LAYERS}
        out["position"] = self.position(s)
        out["config"] = np.array(config_tuple(self.config_of(s)), dtype=np.float64)
        out["own"] = int(sl.own is not None)
        if self.ids is not None:
            out["score clouds"] = np.uint64(sl.clouds)
            out["score counts"] = sl.counts.copy()
        return out

    # -- ops
    def apply(self, op, index=None):
        """what the library must return for `op` (None: nothing to compare); `index`: where the op stands in its list (default: one
        behind the op applied last) -- a cloud op in chained mode names its batch by that"""
        k = op["op"]
        m = self.mutant
        self.at = self.at + 1 if index is None else index
        if "g3" not in op:
            self.mid_seen.append(self.at)
        if k == "checkpoint":
            self.batches.clear()   # (the driver lets go of the batches' device buffers there)
        if k in ("tunings", "synchronize", "batch_fence", "checkpoint"):
            return None
        res = getattr(self, "do_" + k)(op, m)
        self.pred.apply(op)
        return res

    def bind(self, ops):
        """the list the ops come from, for a caller that applies only some of them: a chained cloud call of the second generator stream
        names its batch by its index among the ops that carry no "g3" """
        self.mid = mid_indices(ops)
        return self

    def batch_key(self, src):
        """the index (in the full list) of the batch a chained cloud call names"""
        if src.get("full"):
            return src["batch"]
        table = self.mid if self.mid is not None else self.mid_seen
        return table[src["batch"]] if src["batch"] < len(table) else None

    def run(self, ops):
        self.bind(ops)
        return [self.apply(op, i) for i, op in enumerate(ops)]

    def do_reset_maps(self, op, m):
        for s in range(op["first"], op["first"] + op["n"]):
            sl = self.slots[s]
            old = (sl.ref.layer("ground").copy(), sl.ref.layer("groundpatch").copy()) if m == "fresh_reset_ignored_before_small_batch" else None
            if m == "fresh_map_read_as_before_reset":
                sl.stale_ground = sl.ref.layer("ground").copy()
            self._reset(s, op["pos"], op["odom_z"], op["persistent"])
            sl.stale_gp = old
            if m == "own_config_lost_by_reset_maps":
                sl.own = None

    def do_map_reset(self, op, m):
        self._touch(op["slot"])
        self._reset(op["slot"], op["pos"], op["odom_z"], False)

    def do_move_maps(self, op, m):
        sl = list(op["slots"])
        if m == "move_slots_as_first_plus_i":
            sl = list(range(len(sl)))
        shifts = []
        for s, odom, pose in zip(sl, op["odoms"], op["poses"]):
            shift, before = self._move(s, odom, pose)
            shifts.append(shift)
            if m == "position_not_updated_for_next_batch" and shift != (0, 0):
                self.slots[s].stale_pos = before
            if m == "own_config_lost_by_move_maps" and shift != (0, 0):
                self.slots[s].own = None
        return {"shifts": np.array(shifts, dtype=np.int32).reshape(-1, 2), "fresh maps kept": 1}

    def do_map_move(self, op, m):
        s = op["slot"]
        self._touch(s)
        shift, _ = self._move(s, op["odom"], op["pose"])
        return {"shift": np.array(shift, dtype=np.int32), "position": self.position(s)}

    def do_set_position(self, op, m):
        p = self.slots[op["slot"]].ref._m.contents.position
        self.slots[op["slot"]].prev_pos = (p[0], p[1])
        p[0], p[1] = float(op["pos"][0]), float(op["pos"][1])

    def do_set_layer(self, op, m):
        s = op["slot"]
        sl = self.slots[s]
        self._touch(s)
        if m == "lazy_layers_stale_after_set_layer" and sl.lazy and op["layer"] in LAZY3:
            sl.lazy = False
            return None  # (the values the last cloud left win)
        if op["layer"] in LAZY3:
            sl.lazy = False
        if op["layer"] == "groundpatch" and m != "outlier_walk_skipped_after_set_groundpatch":
            sl.unconfident = False
        if op["layer"] == "ground":
            sl.prev_ground = None
        sl.ref.set_layer(op["layer"], make_layer(op["fill"], op["layer"], self.rows))

    def do_filter_batch(self, op, m):
        slots = list(op["slots"])
        if m == "batch_slots_as_first_plus_i":
            slots = list(range(len(slots)))
        lazy = not self.flags["eager"]
        launch_scores = any(self.slots[s].scoring for s in slots)
        res = {k: [] for k in op["outputs"]}
        rows = self.batches[self.at] = []
        for b, s in enumerate(slots):
            sl = self.slots[s]
            if sl.stale_gp is not None and len(slots) <= 16:
                sl.ref.set_layer("ground", sl.stale_gp[0])
                sl.ref.set_layer("groundpatch", sl.stale_gp[1])
            sl.stale_gp = None
            item = dict(cloud=op["clouds"][b], tf=op["tfs"][b] if op["tfs"] else None)
            in_map = self.map_cloud(item)
            r = self._filter(s, in_map, op["origins"][b], op["base_z"][b], lazy, launch_scores)
            rows.append((in_map, r["label"].copy()))
            emitted = r["index"] >= 0
            k = len(r["out_points"])
            for name in op["outputs"]:
                if name == "labels":
                    res[name].append(r["label"].copy())
                elif name == "out_index":
                    res[name].append(r["index"].copy())
                elif name == "counts":
                    res[name].append(np.array([k] + [int((emitted & (r["cls"] == c)).sum()) for c in (oracle.KEPT, oracle.IGNORED, oracle.OUTLIER)], dtype=np.int32))
                elif name == "out_clouds":
                    res[name].append(r["out_points"].tobytes())
                elif name == "pc2":
                    res[name].append(to_pc2(r["out_points"]).tobytes())
                elif name == "masks":
                    res[name].append(pack_masks(r["label"]))
        return res

    def _single_result(self, r):
        return {"out": r["out_points"].tobytes(), "labels": r["label"].copy(), "index": r["index"].copy()}

    def do_filter_cloud(self, op, m):
        self._touch(op["slot"])
        return self._single_result(self._single(op))

    def do_filter_async2(self, op, m):
        out = {}
        for t, item in enumerate(op["items"]):
            self._touch(item["slot"])
            for key, v in self._single_result(self._single(item)).items():
                out[f"{key} of ticket {t}"] = v
        return out

    def do_filter_layers(self, op, m):
        self._touch(op["slot"])
        out = self._single_result(self._single(op, lazy=False))
        for name in op["layers"]:
            out[f"layer {name}"] = self.slots[op["slot"]].ref.layer(name).copy()
        return out

    def do_filter_pc2(self, op, m):
        self._touch(op["slot"])
        r = self._single(op)
        return {"labels": r["label"].copy(), "index": r["index"].copy(), "returned": len(r["out_points"])}

    def do_filter_pc2_out(self, op, m):
        self._touch(op["slot"])
        # (the record a PointCloud2 payload carries holds x, y, z, intensity, ring: the returned records are built from those)
        return {"records": to_pc2(self._single(op)["out_points"]).tobytes()}

    def do_insert_cloud(self, op, m):
        s = op["slot"]
        sl = self.slots[s]
        self._touch(s)
        sl.ref.cfg = self.config_of(s)
        cls, cell = sl.ref.stage_insert(self.cloud(op["cloud"])[op["start"]: op["end"]], tuple(float(np.float32(v)) for v in op["origin"]))
        sl.last, sl.lazy = None, False
        return {"class": cls.copy(), "cells of the points inside": cell[cls != oracle.OUTSIDE].copy()}

    def do_stage(self, op, m):
        s = op["slot"]
        sl = self.slots[s]
        self._touch(s)
        sl.prev_ground = None
        sl.ref.cfg = self.config_of(s)
        oracle.set_eigen_reduction(0 if m == "eigen_convention_not_applied_to_stage" else self.eigen)
        try:
            st = op["stage"]
            if st == "detect_patches":
                if op["section"] < 0:
                    sl.ref.stage_detect()
                else:
                    sl.ref.stage_detect_section(op["section"])
            elif st == "spiral":
                sl.ref.stage_spiral(op["base_z"])
            elif st in ("patch3", "patch5"):
                sl.ref.detect_ground_patch(3 if st == "patch3" else 5, op["i"], op["j"])
            else:
                sl.ref.interpolate_cell(op["i"], op["j"])
        finally:
            oracle.set_eigen_reduction(0)

    def do_set_config(self, op, m):
        self.cfg = op["cfg"]
        if m == "own_config_lost_by_set_config":
            for sl in self.slots:
                sl.own = None

    def do_set_slot_configs(self, op, m):
        for i, s in enumerate(op["slots"]):
            sl = self.slots[s]
            if op["cfgs"] is None:
                if m == "cleared_slot_keeps_old_context_config" and sl.own is not None:
                    sl.frozen = self.cfg
                sl.own = None
            else:
                sl.own, sl.frozen = op["cfgs"][i], None

    def do_set_conventions(self, op, m):
        self.eigen = op["eigen"]

    def do_set_flags(self, op, m):
        self.flags = dict(minimal=op["minimal"], eager=op["eager"], halves=op["halves"])

    def do_set_score_labels(self, op, m):
        self.ids = list(op["ids"])
        for sl in self.slots:   # "zeroes the counters of every slot (the on / off state of the slots stays)"
            sl.counts[...] = 0
            sl.clouds = 0

    def do_set_scoring(self, op, m):
        if self.ids is None:
            return {"error": "GG_ERR_INVALID"}
        for s in op["slots"]:
            self.slots[s].scoring = bool(op["enable"])

    def do_reset_scores(self, op, m):
        for s in op["slots"]:
            self.slots[s].counts[...] = 0
            self.slots[s].clouds = 0

    def do_get_layer(self, op, m):
        s = op["slot"]
        self._touch(s)
        if op["layer"] in LAZY3:
            self.slots[s].lazy = False
        return {f"layer {op['layer']}": self.slots[s].ref.layer(op["layer"]).copy()}

    def do_get_layers(self, op, m):
        s = op["slot"]
        self._touch(s)
        self.slots[s].lazy = False
        return {f"layer {k}": self.slots[s].ref.layer(k).copy() for k in (op["names"] or LAYERS)}

    def do_export_layers(self, op, m):
        sl = list(op["slots"])
        if m == "export_slots_as_first_plus_i":
            sl = list(range(len(sl)))
        out = {"fresh maps kept": 1}
        if op.get("pad"):
            out["padding untouched"] = 1
        for i, s in enumerate(sl):
            if set(op["names"]) & set(LAZY3):
                self.slots[s].lazy = False
            for k in op["names"]:
                out[f"map {i} (slot {op['slots'][i]}) layer {k}"] = self.slots[s].ref.layer(k).copy()
        return out

    def do_scores(self, op, m):
        if self.ids is None:
            return {"error": "GG_ERR_INVALID"}
        out = {"fresh maps kept": 1}
        for s in op["slots"]:
            out[f"slot {s} clouds"] = np.uint64(self.slots[s].clouds)
            out[f"slot {s} counts"] = self.slots[s].counts.copy()
        return out

    def do_point_classes(self, op, m):
        sl = self.slots[op["slot"]]
        self._touch(op["slot"])
        if sl.last is None or op["n"] is None or len(sl.last[0]) != op["n"]:
            return {"undefined": 1}  # (only in sequences with ops deleted: the header speaks of the slot's last filter call)
        cls, cell = sl.last
        return {"class": cls.copy(), "cells of the points inside": cell[cls != oracle.OUTSIDE].copy()}

    def do_slot_config(self, op, m):
        s = op["slot"]
        return {"config": np.array(config_tuple(self.config_of(s)), dtype=np.float64), "own": int(self.slots[s].own is not None)}

    def do_get_position(self, op, m):
        return {"position": self.position(op["slot"])}

    def do_image_u8(self, op, m):
        s = op["slot"]
        self._touch(s)
        if op["layer"] in LAZY3:
            self.slots[s].lazy = False
        img, lo, hi = image_u8_reference(self.slots[s].ref.layer(op["layer"]))
        return {"image": img, "lower": np.float32(lo), "upper": np.float32(hi)}

    def do_terrain_image(self, op, m):
        s = op["slot"]
        self._touch(s)
        return terrain_reference(self.slots[s].ref.layer("ground"), self.slots[s].ref.layer("pointsRaw"))

    def do_gridmap_message(self, op, m):
        s = op["slot"]
        self._touch(s)
        ref = self.slots[s].ref
        names = op["layers"] or LAYERS
        if set(names) & set(LAZY3):
            self.slots[s].lazy = False
        pos = tuple(ref._m.contents.position)
        return {"message": _gridmap_bytes(ref.rows, ref.cols, ref.resolution, ref.length, pos, [(k, ref.layer(k)) for k in names], tuple(op["stamp"]),
                                          seq=op["seq"])}

    # -- the many-map calls (include/groundgrid_hip.h: gg_import_layers, gg_export_images, gg_export_slopes, gg_split_clouds, ...)
    def do_import_layers(self, op, m):
        """what gg_set_layer of every named layer of every listed map would leave"""
        slots = list(op["slots"])
        if m == "import_slots_as_first_plus_i":
            slots = list(range(len(slots)))
        names = list(op["names"])
        for i, s in enumerate(slots):
            sl = self.slots[s]
            self._touch(s)
            skip = set()
            if m == "import_leaves_fresh_map_fresh" and self.pred.state["fresh"][s]:
                skip = {"ground", "groundpatch"}
            if m == "import_drops_lazy_layers" and sl.lazy and sl.prev3 and set(names) & set(PER_CALL):
                for k in LAZY3:
                    sl.ref.set_layer(k, sl.prev3[k])
            if set(names) & set(PER_CALL):
                sl.lazy = False
            if "groundpatch" in names and m != "import_groundpatch_keeps_no_confidence":
                sl.unconfident = False
            if "ground" in names:
                sl.prev_ground = None
            for k in names:
                if k not in skip:
                    sl.ref.set_layer(k, make_layer(op["fills"][i], k, self.rows))
        return {"fresh maps as the header says": 1}

    @contextlib.contextmanager
    def _as_read(self, s, cloud_reader):
        """(mutants) the slot as a wrong library would see it while a reader runs: put back afterwards"""
        sl, m = self.slots[s], self.mutant
        p = sl.ref._m.contents.position
        pos = ground = None
        if cloud_reader and m == "cloud_reader_position_before_last_move" and sl.prev_pos is not None:
            pos, (p[0], p[1]) = (p[0], p[1]), sl.prev_pos
        stale = None
        if cloud_reader and m == "cloud_reader_ground_before_last_scroll" and sl.prev_ground is not None:
            stale = sl.prev_ground
        if m == "fresh_map_read_as_before_reset" and sl.stale_ground is not None and self.pred.state["fresh"][s]:
            stale = sl.stale_ground
        if stale is not None:
            ground = sl.ref.layer("ground").copy()
            sl.ref.set_layer("ground", stale)
        try:
            yield sl.ref
        finally:
            if pos is not None:
                p[0], p[1] = pos
            if ground is not None:
                sl.ref.set_layer("ground", ground)

    def do_export_images(self, op, m):
        out = {"fresh maps kept": 1, "nothing else written": 1}
        for i, s in enumerate(op["slots"]):
            sl = self.slots[s]
            with self._as_read(s, False) as ref:
                for k in op["names"]:
                    L = ref.layer(k)
                    if m == "images_read_lazy_layer_uncomputed" and sl.lazy and sl.prev3 and k in LAZY3:
                        L = sl.prev3[k]
                    if np.isfinite(L).any():
                        img, lo, hi = image_u8_reference(L)
                    else:
                        img, lo, hi = np.zeros(L.shape, np.uint8), np.float32(np.inf), np.float32(-np.inf)
                    out[f"map {i} (slot {s}) image {k}"] = np.ascontiguousarray(img)
                    if op["bounds"]:
                        out[f"map {i} (slot {s}) bounds {k}"] = np.array([lo, hi], dtype=np.float32)
                if op["terrain"]:
                    for key, v in terrain_reference(ref.layer("ground"), ref.layer("pointsRaw")).items():
                        out[f"map {i} (slot {s}) terrain {key}"] = v
            if set(op["names"]) & set(LAZY3):
                sl.lazy = False
        return out

    def do_export_slopes(self, op, m):
        out = {"fresh maps kept": 1, "lazy maps kept": 1, "nothing else written": 1}
        for i, s in enumerate(op["slots"]):
            with self._as_read(s, False) as ref:
                planes = _memo(("slopes", _digest(ref.layer("ground")), _digest(ref.layer("groundpatch")), self.shape),
                               lambda: slopes_ref.slopes_reference(ref.layer("ground"), ref.layer("groundpatch"), np.float32(self.sh["res"])))
            for k in op["channels"]:
                out[f"map {i} (slot {s}) {k}"] = planes[SLOPE_CHANNELS.index(k)]
        return out

    def _labelled(self, op):
        """per listed cloud (slot, the points in the map frame, one label byte per point), or None: a chained op whose batch is not there
        (a list with ops deleted)"""
        src = op["source"]
        if src["mode"] == "chained":
            rows = self.batches.get(self.batch_key(src))
            if rows is None or len(rows) < src["row0"] + len(op["slots"]):
                return None
            return [(s,) + rows[src["row0"] + i] for i, s in enumerate(op["slots"])]
        out = []
        for i, s in enumerate(op["slots"]):
            c = self.map_cloud(dict(cloud=src["clouds"][i], tf=src["tfs"][i] if src["tfs"] else None))
            out.append((s, c, foreign_labels(src["labels"], i, len(c))))
        return out

    def _cloud_call(self, op, m, expect):
        clouds = self._labelled(op)
        if clouds is None:
            return {"undefined": 1}
        out = {"fresh maps kept": 1, "lazy maps kept": 1, "nothing else written": 1}
        params = json.dumps({k: v for k, v in op.items() if k not in ("slots", "source", "stream", "origins")}, sort_keys=True)
        for i, (s, cloud, labels) in enumerate(clouds):
            with self._as_read(s, True) as ref:
                key = (params, json.dumps(op["origins"][i]) if "origins" in op else "", self.shape, tuple(ref._m.contents.position),
                       _digest(ref.layer("ground")), _digest(cloud), _digest(labels))
                res = _memo(key, lambda: expect(i, ref, cloud, labels))
            if m == "foreign_point_outside_gets_finite_height" and op["source"]["mode"] == "foreign":
                res = {k: (np.where(np.isnan(v), np.float32(0.0), v) if k.endswith("height") else v) for k, v in res.items()}
            for k, v in res.items():
                out[f"cloud {i} (slot {s}) {k}"] = v
                if k in ("state", "cell ids", "point ids", "clusters", "dist2"):   # (what a plane call or one of tests/seq_late.py may be chained to)
                    self.outs.setdefault(self.at, {"_op": op}).setdefault(k, []).append(v)
        return out

    def do_split_clouds(self, op, m):
        def expect(i, ref, cloud, labels):
            res = {}
            sets = cloud_refs.expected_sets(ref, cloud, labels)
            for name in cloud_refs.SETS:
                idx, recs, h = sets[name]
                res[f"{name} count"] = np.int32(len(idx))
                for field in op["want"].get(name, []):
                    res[f"{name} {field}"] = {"points": np.frombuffer(recs.tobytes(), dtype=np.uint32).reshape(-1, 4), "height": h, "source": idx}[field]
            return res

        return self._cloud_call(op, m, expect)

    def do_rasterize_clouds(self, op, m):
        def expect(i, ref, cloud, labels):
            planes = cloud_refs.expected_planes(ref, cloud, labels)
            return {k: planes[RASTER_CHANNELS.index(k)] for k in op["channels"]}

        return self._cloud_call(op, m, expect)

    @staticmethod
    def _band(op):
        return (-np.inf if op["min_height"] is None else op["min_height"]), (np.inf if op["max_height"] is None else op["max_height"])

    def do_cluster_clouds(self, op, m):
        def expect(i, ref, cloud, labels):
            lo, hi = self._band(op)
            plane, K, table, ids = cloud_refs.expected_clusters(ref, cloud, labels, op["min_points"], lo, hi, op["connectivity"],
                                                                "row" if op["row_major"] else "col")
            res = {"cell ids": plane, "clusters": np.int32(K)}
            if op["max_clusters"]:
                res["table"] = table[: min(K, op["max_clusters"])]
            if op["point_clusters"]:
                res["point ids"] = ids
            return res

        return self._cloud_call(op, m, expect)

    def do_clearance_clouds(self, op, m):
        def expect(i, ref, cloud, labels):
            lo, hi = self._band(op)
            occupied = cloud_refs.occupied_cells(ref, cloud, labels, op["min_points"], lo, hi)
            if op["nearest"]:
                dist2, nearest, distance, count = clearance_ref.expected_clearance(occupied, op["max_cells"], "row" if op["row_major"] else "col", self.sh["res"])
            else:
                dist2, distance, count = cloud_refs.expected_clearance_fast(occupied, op["max_cells"], self.sh["res"])
            res = {"dist2": dist2, "occupied cells": np.int32(count)}
            if op["nearest"]:
                res["nearest"] = nearest
            if op["distance"]:
                res["distance bits"] = distance
            return res

        return self._cloud_call(op, m, expect)

    def do_visibility_clouds(self, op, m):
        def expect(i, ref, cloud, labels):
            lo, hi = self._band(op)
            state, counts = cloud_refs.expected_visibility(ref, cloud, labels, op["origins"][i][:2], op["min_points"], lo, hi, op["max_cells"], "row")
            res = {"state": state}
            if op["counts"]:
                res["counts"] = counts
            return res

        return self._cloud_call(op, m, expect)


for _kind in PLANE_KINDS:
    setattr(ContextModel, "do_" + _kind, lambda self, op, m: seq_planes.model_op(self, op, m))
for _kind in LATE_KINDS:
    setattr(ContextModel, "do_" + _kind, lambda self, op, m: seq_late.model_op(self, op, m))

_MEMO = {}


def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest()


def _memo(key, compute):
    """the expectation of a reader is a pure function of the planes, the position, the points, the labels and the op's data: the tests run
    the model many times (once per mutant) over mostly the same states"""
    if key not in _MEMO:
        if len(_MEMO) > 4000:
            _MEMO.clear()
        _MEMO[key] = compute()
    return _MEMO[key]


def foreign_labels(spec, i, n):
    """the label bytes of cloud i of a foreign source: {"seed"}; ground, non-ground and bytes that select nothing"""
    rng = np.random.default_rng([int(spec["seed"]), i, 79])
    return rng.choice(np.array([49, 99, 99, 49, 0, 7, 98, 255], dtype=np.uint8), n)


# ---------------------------------------------------------------------------------------------------------------- the driver

class DeviceFault(Exception):
    """GG_ERR_HIP or a pending gg_device_error: nothing more may be started on the card"""


class _Null:
    """an output the batch does not ask for (a null pointer in gg_batch)"""

    @staticmethod
    def data_ptr():
        return None


def api_config(index):
    from groundgrid_amd import api

    c = api.default_config()
    for k, v in CONFIGS[index].items():
        setattr(c, k, v)
    return c


def create_context(shape):
    from groundgrid_amd import api

    sh = SHAPES[shape]
    return api.GroundSegmentation().init(sh["length"], sh["res"], n_slots=sh["n_slots"], max_points=sh["stride"])


class Driver:
    """Issues ops through groundgrid_amd.api.  `on_result(i, got)` is called once per op, in op order, as soon as the op's results may
    be looked at: at once while nothing enqueued earlier is still pending, otherwise at the next checkpoint."""

    def __init__(self, seg, shape, on_result=None):
        import torch

        self.torch, self.seg, self.shape, self.sh = torch, seg, shape, SHAPES[shape]
        self.on_result = on_result or (lambda i, got: None)
        self.streams = {"default": None, "s1": torch.cuda.Stream(), "s2": torch.cuda.Stream()}
        self.pending = []          # [(op index, thunk -> result)] in op order
        self.used = set()          # caller streams with work enqueued since the last checkpoint
        self.keep = []             # device tensors that must outlive the enqueued work
        self._clouds = {}
        self.planes = {}
        self.batches = {}          # op index of a filter_batch -> its device buffers, until the next checkpoint (chained cloud calls)
        self.at = -1
        self.dev_outs = {}         # op index -> {output name: (tensor, stride in words, maps, row_major)}: what a plane call may be chained to
        self.chain_bufs = {}       # (chain, name, which of the two) -> the chain's own device buffer; both outlive checkpoints
        self.shift_log = []        # (op index, slot, shift as the library returned it) of every move
        self.mid = []

    def cloud(self, spec):
        return cached_cloud(spec, self.shape)

    def handle(self, name):
        """the stream handle as api.py takes it: None = the context's own; 0 = torch's default stream"""
        if name == "ctx":
            return None
        st = self.streams[name]
        return 0 if st is None else st.cuda_stream

    def on(self, name):
        st = self.streams.get(name)
        return self.torch.cuda.stream(st) if st is not None else _NoContext()

    def fresh_count(self):
        return self.seg.debug_set_tuning("fresh_count", 0)

    def check_device(self):
        if self.seg._L.gg_device_error(self.seg._ctx, 0) != 0:
            raise DeviceFault("gg_device_error reports a wait that ran out")

    def flush(self, force=False):
        while self.pending and (force or not self.pending[0][2]):
            i, thunk, _ = self.pending.pop(0)
            self.on_result(i, thunk())

    def run(self, ops):
        from groundgrid_amd import api

        self.mid = mid_indices(ops)
        for i, op in enumerate(ops):
            self.at = i
            try:
                got = getattr(self, "do_" + op["op"])(op)
            except api.GroundGridError as e:
                if "GG_ERR_HIP" in str(e) or "HIP" in str(e):
                    raise DeviceFault(str(e))
                raise
            if callable(got):
                self.pending.append((i, got, True))
            else:
                self.pending.append((i, (lambda g=got: g), False))
            self.flush()
        assert not self.pending, "a sequence ends with a checkpoint"

    # -- ops
    def do_tunings(self, op):
        for key in ("graphs", "halves_min_clouds", "front", "sweep_waves", "scan_parts", "move_chunk", "export_variant"):
            if key == "halves_min_clouds" and not op[key]:
                continue
            self.seg.debug_set_tuning(key, op[key])

    def do_checkpoint(self, op):
        for name in sorted(self.used):
            self.seg.batch_fence(stream=self.handle(name))
        self.used.clear()
        self.torch.cuda.synchronize()
        self.check_device()
        self.flush(force=True)
        self.keep.clear()
        self.batches.clear()

    def do_synchronize(self, op):
        self.seg.synchronize()

    def do_batch_fence(self, op):
        self.seg.batch_fence(stream=self.handle(op["stream"]))

    def do_reset_maps(self, op):
        with self.on(op["stream"]):
            self.seg.reset_maps(op["first"], op["n"], odom_z=op["odom_z"], pos=op["pos"], persistent_only=op["persistent"],
                                on_torch_stream=op["stream"] != "ctx")
        if op["stream"] != "ctx":
            self.used.add(op["stream"])

    def do_map_reset(self, op):
        self.seg.map(op["slot"]).reset(odom_z=op["odom_z"], pos=op["pos"])

    def do_move_maps(self, op):
        before = self.fresh_count()
        shifts = self.seg.move_maps(op["odoms"], op["poses"], slots=op["slots"], stream=self.handle(op["stream"]))
        for s, sh in zip(op["slots"], np.asarray(shifts).reshape(-1, 2)):
            self.shift_log.append((self.at, s, (int(sh[0]), int(sh[1]))))
        if op["stream"] != "ctx":
            self.used.add(op["stream"])
        # (a fresh map that scrolls is written; every other fresh map of the context stays fresh, and so does one whose shift is (0, 0))
        return {"shifts": shifts, "fresh maps kept": int(self.fresh_count() >= before - int(np.count_nonzero(np.any(shifts != 0, axis=1))))}

    def do_map_move(self, op):
        m = self.seg.map(op["slot"])
        shift = m.move(op["odom"][0], op["odom"][1], op["pose"])
        self.shift_log.append((self.at, op["slot"], (int(shift[0]), int(shift[1]))))
        return {"shift": np.array(shift, dtype=np.int32), "position": np.array(m.getPosition(), dtype=np.float64)}

    def do_set_position(self, op):
        self.seg.map(op["slot"]).setPosition(*op["pos"])

    def do_set_layer(self, op):
        self.seg.map(op["slot"]).set(op["layer"], make_layer(op["fill"], op["layer"], self.seg.rows))

    def do_filter_batch(self, op):
        from groundgrid_amd import api

        torch, B, stride = self.torch, len(op["slots"]), self.sh["stride"]
        clouds = [self.cloud(c) for c in op["clouds"]]
        if op["fmt"] == 16:
            host = np.zeros((B, stride), dtype=api.POINT16_DTYPE)
            for b, c in enumerate(clouds):
                host[b, : len(c)] = api.pack16(c)
            raw = host.view(np.uint8).reshape(B, stride, 16)
        else:
            raw = np.zeros((B, stride, 32), dtype=np.uint8)
            for b, c in enumerate(clouds):
                raw[b, : len(c)] = np.frombuffer(c.tobytes(), dtype=np.uint8).reshape(-1, 32)
        want = set(op["outputs"])
        own = op["stream"] == "ctx"
        with self.on(op["stream"]):   # (the upload, the output buffers' fills and the batch on one stream: no synchronisation anywhere)
            dev = torch.device("cuda", self.seg.device)
            staged = torch.from_numpy(raw).pin_memory()   # (pinned: the copy is enqueued, the host does not wait for the stream)
            pts = staged.to(dev, non_blocking=True)
            out = api.BatchOutputs(
                labels=torch.full((B, stride), 0xEE, dtype=torch.uint8, device=dev) if "labels" in want else _Null,
                out_index=torch.full((B, stride), -77, dtype=torch.int32, device=dev) if "out_index" in want else _Null,
                counts=torch.full((B, 4), -77, dtype=torch.int32, device=dev) if "counts" in want else _Null,
                out_clouds=torch.zeros((B, stride, 32), dtype=torch.uint8, device=dev) if "out_clouds" in want else None,
                label_masks=torch.zeros((B, stride // 4), dtype=torch.uint8, device=dev) if "masks" in want else None,
                out_pc2=torch.zeros((B, stride * 18), dtype=torch.uint8, device=dev) if "pc2" in want else None)
            tfs = None
            if op["tfs"]:
                tfs = np.stack([api.transform_from_pose(p, "kdl") for p in op["tfs"]])
            if own:   # the context's own stream is no torch stream: the inputs, enqueued on torch's current one, have to be there first
                torch.cuda.current_stream(dev).synchronize()
            self.seg.filter_batch(pts, [len(c) for c in clouds], op["origins"], op["base_z"], out=out, transforms=tfs, slots=op["slots"],
                                  stream=self.handle(op["stream"]), own_stream=own)
        if not own:
            self.used.add(op["stream"])
        self.keep.append((staged, pts, out))
        n = [len(c) for c in clouds]
        self.batches[self.at] = (pts, out, n, tfs)

        def collect():
            res = {}
            if "labels" in want:
                a = out.labels.cpu().numpy()
                res["labels"] = [a[b, : n[b]] for b in range(B)]
            if "out_index" in want:
                a = out.out_index.cpu().numpy()
                res["out_index"] = [a[b, : n[b]] for b in range(B)]
            if "counts" in want:
                a = out.counts.cpu().numpy()
                res["counts"] = [a[b] for b in range(B)]
            # (the sizes of the returned clouds come from the model where the batch did not ask for the counts: the rows are compared
            # over the length the model expects either way)
            if "masks" in want:
                a = out.label_masks.cpu().numpy()
                res["masks"] = [a[b, : (n[b] + 3) // 4] for b in range(B)]
            if "out_clouds" in want:
                a = out.out_clouds.cpu().numpy()
                res["out_clouds"] = [a[b].tobytes() for b in range(B)]
            if "pc2" in want:
                a = out.out_pc2.cpu().numpy()
                res["pc2"] = [a[b].tobytes() for b in range(B)]
            return res

        return collect

    def _single_args(self, item):
        from groundgrid_amd import api

        tf = None if item.get("tf") is None else api.transform_from_pose(item["tf"], "kdl")
        return self.cloud(item["cloud"]), item["origin"], item["base_z"], self.seg.map(item["slot"]), tf

    def do_filter_cloud(self, op):
        c, org, bz, m, tf = self._single_args(op)
        out, labels, index = self.seg.filter_cloud(c, org, bz, map=m, return_details=True, map_from_cloud=tf)
        return {"out": out.tobytes(), "labels": labels, "index": index}

    def do_filter_async2(self, op):
        tickets = []
        for item in op["items"]:
            c, org, bz, m, tf = self._single_args(item)
            tickets.append(self.seg.filter_cloud_async(c, org, bz, map=m, map_from_cloud=tf))
        res = {}
        for t, ticket in enumerate(tickets):
            out, labels, index = self.seg.filter_cloud_wait(ticket, return_details=True)
            res[f"out of ticket {t}"], res[f"labels of ticket {t}"], res[f"index of ticket {t}"] = out.tobytes(), labels.copy(), index.copy()
        return res

    def do_filter_layers(self, op):
        c, org, bz, m, tf = self._single_args(op)
        key = bool(op["registered"])
        if key not in self.planes:
            self.planes[key] = self.seg.alloc_layers(register=key)
        use = {k: self.planes[key][k] for k in op["layers"]}
        for v in use.values():
            v[...] = np.float32(-7.0)
        out, labels, index = self.seg.filter_cloud_with_layers(c, org, bz, use, map=m, return_details=True, map_from_cloud=tf)
        res = {"out": out.tobytes(), "labels": labels, "index": index}
        for k, v in use.items():
            res[f"layer {k}"] = v.copy()
        return res

    def do_filter_pc2(self, op):
        c, org, bz, m, tf = self._single_args(op)
        labels, index, k = self.seg.filter_cloud_pc2(to_pc2(c).tobytes(), len(c), 18, (0, 4, 8, 16), org, bz, map=m, map_from_cloud=tf)
        return {"labels": labels, "index": index, "returned": k}

    def do_filter_pc2_out(self, op):
        c, org, bz, m, tf = self._single_args(op)
        rec = self.seg.filter_cloud_pc2_out(to_pc2(c).tobytes(), len(c), 18, (0, 4, 8, 16), org, bz, map=m, map_from_cloud=tf)
        return {"records": rec.tobytes()}

    def do_insert_cloud(self, op):
        cls, cell = self.seg.map(op["slot"]).insert_cloud(self.cloud(op["cloud"]), op["start"], op["end"], op["origin"])
        return {"class": cls, "cells of the points inside": cell[cls != 0]}

    def do_stage(self, op):
        m, st = self.seg.map(op["slot"]), op["stage"]
        if st == "detect_patches":
            m.detect_ground_patches(op["section"])
        elif st == "spiral":
            m.spiral_ground_interpolation(op["base_z"])
        elif st in ("patch3", "patch5"):
            m.detect_ground_patch(3 if st == "patch3" else 5, op["i"], op["j"])
        else:
            m.interpolate_cell(op["i"], op["j"])

    def do_set_config(self, op):
        self.seg.setConfig(api_config(op["cfg"]))

    def do_set_slot_configs(self, op):
        self.seg.set_slot_configs(None if op["cfgs"] is None else [api_config(i) for i in op["cfgs"]], slots=op["slots"])

    def do_set_conventions(self, op):
        self.seg.set_conventions(eigen_reduction=op["eigen"])

    def do_set_flags(self, op):
        self.seg.set_flags(minimal_layers=op["minimal"], eager_layers=op["eager"], concurrent_halves=op["halves"])

    def do_set_score_labels(self, op):
        self.seg.set_score_labels(op["ids"])

    def do_set_scoring(self, op):
        self.seg.set_scoring(slots=op["slots"], enable=op["enable"])

    def do_reset_scores(self, op):
        self.seg.reset_scores(slots=op["slots"])

    def do_get_layer(self, op):
        return {f"layer {op['layer']}": self.seg.map(op["slot"]).get(op["layer"])}

    def do_get_layers(self, op):
        return {f"layer {k}": v for k, v in self.seg.map(op["slot"]).layers(op["names"]).items()}

    def do_export_layers(self, op):
        torch = self.torch
        before = self.fresh_count()
        own, pad = op["stream"] == "ctx", int(op.get("pad") or 0)
        cells, n, K = self.seg.rows * self.seg.cols, len(op["slots"]), len(op["names"])
        with self.on(op["stream"]):
            kw = {}
            if pad:   # planes further apart than they are long: the floats between them keep the sentinel
                kw = dict(plane_stride=cells + pad,
                          out=torch.full((n * K * (cells + pad),), 0x7FC12345, dtype=torch.int32, device=torch.device("cuda", self.seg.device)).view(torch.float32))
                if own:
                    torch.cuda.current_stream(self.seg.device).synchronize()
            t = self.seg.export_layers(op["names"], slots=op["slots"], row_major=op["row_major"], stream=self.handle(op["stream"]), own_stream=own, **kw)
        kept = int(self.fresh_count() == before)
        if not own:
            self.used.add(op["stream"])
        self.keep.append(t)
        shape = (n, K, self.seg.rows, self.seg.cols) if op["row_major"] else (n, K, self.seg.cols, self.seg.rows)

        def collect():
            a = t.cpu().numpy()
            res = {"fresh maps kept": kept}
            if pad:
                a = a.reshape(n, K, cells + pad)
                res["padding untouched"] = int(np.all(a[:, :, cells:].view(np.uint32) == 0x7FC12345))
                a = a[:, :, :cells]
            a = a.reshape(shape)
            for i, s in enumerate(op["slots"]):
                for k, name in enumerate(op["names"]):
                    res[f"map {i} (slot {s}) layer {name}"] = a[i, k] if op["row_major"] else a[i, k].T
            return res

        return collect

    def do_scores(self, op):
        before = self.fresh_count()
        clouds, counts = self.seg.scores_raw(slots=op["slots"])
        res = {"fresh maps kept": int(self.fresh_count() == before)}
        for i, s in enumerate(op["slots"]):
            res[f"slot {s} clouds"], res[f"slot {s} counts"] = np.uint64(clouds[i]), counts[i]
        return res

    def do_point_classes(self, op):
        cls, cell = self.seg.point_classes(op["n"], map=self.seg.map(op["slot"]))
        return {"class": cls, "cells of the points inside": cell[cls != 0]}

    def do_slot_config(self, op):
        c, own = self.seg.slot_config(op["slot"])
        return {"config": np.array(config_tuple(c), dtype=np.float64), "own": int(own)}

    def do_get_position(self, op):
        return {"position": np.array(self.seg.map(op["slot"]).getPosition(), dtype=np.float64)}

    def library_position(self, slot):
        """gg_get_map_position itself, next to the handle's own record of it"""
        import ctypes as C

        x, y = C.c_double(), C.c_double()
        self.seg._L.gg_get_map_position(self.seg._ctx, slot, C.byref(x), C.byref(y))
        return np.array([x.value, y.value], dtype=np.float64)

    def do_image_u8(self, op):
        img, lo, hi = self.seg.map(op["slot"]).image_u8(op["layer"])
        return {"image": img, "lower": np.float32(lo), "upper": np.float32(hi)}

    def do_terrain_image(self, op):
        t = self.seg.map(op["slot"]).terrain_image()
        return {"ground": t[:, :, 0], "raw": t[:, :, 2], "visited": t[1:-1, 1:-1, 1]}

    def do_gridmap_message(self, op):
        return {"message": self.seg.map(op["slot"]).gridmap_message(layers=op["layers"], seq=op["seq"], stamp=tuple(op["stamp"]))}

    # -- the many-map calls: sentinel-filled destinations with SLACK words behind them, everything compared on bits at the next checkpoint
    SLACK = 5

    def _stream_arg(self, name):
        return self.seg._stream_arg(name != "ctx", handle=self.handle(name))

    def _dev(self):
        return self.torch.device("cuda", self.seg.device)

    def _words(self, count):
        return self.torch.full((count + self.SLACK,), SENTINEL, dtype=self.torch.int32, device=self._dev())

    def _upload(self, host):
        staged = self.torch.from_numpy(np.ascontiguousarray(host)).pin_memory()   # (pinned: enqueued, the host does not wait)
        dev = staged.to(self._dev(), non_blocking=True)
        self.keep.append((staged, dev))
        return dev

    def _marks(self):
        return self.fresh_count(), self.seg.debug_set_tuning("lazy_count", 0)

    def _enqueue(self, op, call):
        """the C call on the op's stream; returns what the host-side marks did: (fresh maps before, after, lazy maps before, after)"""
        from groundgrid_amd import api

        if op["stream"] == "ctx":   # the context's own stream is no torch stream: the inputs and the fills have to be there first
            self.torch.cuda.current_stream(self.seg.device).synchronize()
        else:
            self.used.add(op["stream"])
        before = self._marks()
        api._check(self.seg._L, self.seg._ctx, call(self._stream_arg(op["stream"])), "gg_" + op["op"])
        after = self._marks()
        return before[0], after[0], before[1], after[1]

    def _planes(self, a, n, K, stride, row_major):
        """the n * K planes of a downloaded destination as [rows, cols] arrays, and whether every other word still holds the sentinel"""
        rows, cols = self.seg.rows, self.seg.cols
        cells = rows * cols
        body = a[: n * K * stride].reshape(n * K, stride)
        clean = bool(np.all(body[:, cells:].view(np.uint32) == SENTINEL) and np.all(a[n * K * stride:].view(np.uint32) == SENTINEL))
        planes = [p[:cells].reshape(rows, cols) if row_major else p[:cells].reshape((rows, cols), order="F") for p in body]
        return planes, clean

    def do_import_layers(self, op):
        torch, rows, cols = self.torch, self.seg.rows, self.seg.cols
        n, K, stride = len(op["slots"]), len(op["names"]), rows * cols + int(op["pad"])
        host = np.full(n * K * stride + self.SLACK, SENTINEL, dtype=np.uint32).view(np.float32)
        for i in range(n):
            for k, name in enumerate(op["names"]):
                plane = make_layer(op["fills"][i], name, rows)
                host[(i * K + k) * stride: (i * K + k) * stride + rows * cols] = plane.ravel(order="C" if op["row_major"] else "F")
        own = op["stream"] == "ctx"
        with self.on(op["stream"]):
            src = self._upload(host)
            if own:
                torch.cuda.current_stream(self.seg.device).synchronize()
            else:
                self.used.add(op["stream"])
            f0 = self.fresh_count()
            self.seg.import_layers(src[: n * K * stride], op["names"], slots=op["slots"], row_major=op["row_major"], stream=self.handle(op["stream"]),
                                   own_stream=own, plane_stride=stride)
            f1 = self.fresh_count()
        # (a fresh map whose mask names neither ground nor groundpatch, and every map that is not listed, stays fresh)
        return {"fresh maps as the header says": int(f1 == f0 if not set(op["names"]) & {"ground", "groundpatch"} else f0 - n <= f1 <= f0)}

    def do_export_slopes(self, op):
        rows, cols = self.seg.rows, self.seg.cols
        n, K, stride = len(op["slots"]), len(op["channels"]), rows * cols + int(op["pad"])
        own = op["stream"] == "ctx"
        with self.on(op["stream"]):
            dst = self._words(n * K * stride)
            if own:
                self.torch.cuda.current_stream(self.seg.device).synchronize()
            else:
                self.used.add(op["stream"])
            before = self._marks()
            self.seg.export_slopes(op["channels"], slots=op["slots"], out=dst[: n * K * stride].view(self.torch.float32), row_major=op["row_major"],
                                   stream=self.handle(op["stream"]), own_stream=own, plane_stride=stride)
            after = self._marks()
        self.keep.append(dst)

        def collect():
            planes, clean = self._planes(dst.cpu().numpy(), n, K, stride, op["row_major"])
            res = {"fresh maps kept": int(before[0] == after[0]), "lazy maps kept": int(before[1] == after[1]), "nothing else written": int(clean)}
            for i, s in enumerate(op["slots"]):
                for k, name in enumerate(op["channels"]):
                    res[f"map {i} (slot {s}) {name}"] = planes[i * K + k].view(np.float32)
            return res

        return collect

    def do_export_images(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        torch, rows, cols = self.torch, self.seg.rows, self.seg.cols
        cells, n, K, pad = rows * cols, len(op["slots"]), len(op["names"]), int(op["pad"])
        with self.on(op["stream"]):
            images = torch.full((n * K * (cells + pad) + self.SLACK,), 0xA5, dtype=torch.uint8, device=self._dev()) if K else None
            bounds = self._words(n * K * 2) if K and op["bounds"] else None
            terrain = self._words(n * (3 * cells + pad)) if op["terrain"] else None
            x = _lib.GGImageExport()
            sl = (C.c_int32 * n)(*op["slots"])
            x.n, x.first_slot, x.slots = n, 0, sl
            x.layer_mask = sum(1 << LAYERS.index(k) for k in op["names"])
            x.d_images, x.image_stride = (images.data_ptr() if K else None), cells + pad
            x.d_bounds = bounds.data_ptr() if bounds is not None else None
            x.d_terrain, x.terrain_stride = (terrain.data_ptr() if op["terrain"] else None), 3 * cells + pad
            x.terrain_layout = _lib.GG_TERRAIN_CHW if op["chw"] else _lib.GG_TERRAIN_HWC
            marks = self._enqueue(op, lambda st: self.seg._L.gg_export_images(self.seg._ctx, C.byref(x), st))
        self.keep.append((images, bounds, terrain))

        def collect():
            res = {"fresh maps kept": int(marks[0] == marks[1])}
            clean = True
            if K:
                a = images.cpu().numpy()
                body = a[: n * K * (cells + pad)].reshape(n * K, cells + pad)
                clean &= bool(np.all(body[:, cells:] == 0xA5) and np.all(a[n * K * (cells + pad):] == 0xA5))
                if bounds is not None:
                    b = bounds.cpu().numpy()
                    clean &= bool(np.all(b[n * K * 2:].view(np.uint32) == SENTINEL))
            if op["terrain"]:
                t = terrain.cpu().numpy()
                tb = t[: n * (3 * cells + pad)].reshape(n, 3 * cells + pad)
                clean &= bool(np.all(tb[:, 3 * cells:].view(np.uint32) == SENTINEL) and np.all(t[n * (3 * cells + pad):].view(np.uint32) == SENTINEL))
            for i, s in enumerate(op["slots"]):
                for k, name in enumerate(op["names"]):
                    res[f"map {i} (slot {s}) image {name}"] = body[i * K + k, :cells].reshape(rows, cols)
                    if bounds is not None:
                        res[f"map {i} (slot {s}) bounds {name}"] = b[(i * K + k) * 2: (i * K + k) * 2 + 2].view(np.float32)
                if op["terrain"]:
                    img = tb[i, : 3 * cells].view(np.float32)
                    ch = img.reshape(3, rows, cols) if op["chw"] else np.moveaxis(img.reshape(rows, cols, 3), 2, 0)
                    res[f"map {i} (slot {s}) terrain ground"], res[f"map {i} (slot {s}) terrain raw"] = ch[0], ch[2]
                    res[f"map {i} (slot {s}) terrain visited"] = ch[1][1:-1, 1:-1]
            res["nothing else written"] = int(clean)
            return res

        return collect

    def _cloud_source(self, op, x):
        """the ten leading members of a gg_cloud_* structure `x`; returns (n_points per cloud, cloud_stride, what has to stay referenced
        until the C call has returned)"""
        import ctypes as C

        from groundgrid_amd import _lib, api

        src, n = op["source"], len(op["slots"])
        if src["mode"] == "chained":   # the batch's own device buffers, wherever that batch stands in its stream
            pts, out, n_pts, tfs = self.batches[src["batch"] if src.get("full") else self.mid[src["batch"]]]
            rec, stride, row0 = int(pts.shape[2]), int(pts.shape[1]), src["row0"]
            d_points = pts.data_ptr() + row0 * stride * rec
            n_pts = n_pts[row0: row0 + n]
            tfs = None if tfs is None else tfs[row0: row0 + n]
            labels = None if op["masks"] else out.labels.data_ptr() + row0 * stride
            masks = out.label_masks.data_ptr() + row0 * (stride // 4) if op["masks"] else None
        else:
            rec, stride = src["fmt"], src["stride"]
            clouds = [self.cloud(c) for c in src["clouds"]]
            n_pts = [len(c) for c in clouds]
            raw = np.zeros((n, stride, rec), dtype=np.uint8)
            lab = np.full((n, stride), 99, dtype=np.uint8)   # (behind a cloud's end: non-ground points at the origin, for a kernel that reads too far)
            for i, c in enumerate(clouds):
                raw[i, : len(c)] = np.frombuffer((api.pack16(c) if rec == 16 else c).tobytes(), dtype=np.uint8).reshape(-1, rec)
                lab[i, : len(c)] = foreign_labels(src["labels"], i, len(c))
            if op["masks"]:
                code = np.where(lab == 49, 1, np.where(lab == 99, 2, 0)).astype(np.uint8).reshape(n, stride // 4, 4)
                lab = (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)
            d_points = self._upload(raw).data_ptr()
            given = self._upload(lab).data_ptr()
            labels, masks = (None, given) if op["masks"] else (given, None)
            tfs = None if not src["tfs"] else np.stack([api.transform_from_pose(p, "kdl") for p in src["tfs"]])
        keep = [(C.c_int32 * n)(*op["slots"]), (C.c_int32 * n)(*[int(v) for v in n_pts])]
        x.n, x.first_slot, x.slots, x.point_format = n, 0, keep[0], _lib.GG_POINT16 if rec == 16 else _lib.GG_POINT32
        x.d_points, x.cloud_stride, x.n_points = d_points, stride, keep[1]
        if tfs is not None:
            keep.append(np.ascontiguousarray(np.asarray(tfs, dtype=np.float64).reshape(n, 12)))
            x.transforms = keep[-1].ctypes.data_as(C.POINTER(C.c_double))
        x.d_labels, x.d_label_masks = labels, masks
        self.last_points = dict(ptr=d_points, stride=stride, n_points=list(n_pts), rec=rec, tfs=tfs)   # (gg_box_clusters runs on the same points)
        return n_pts, stride, keep

    @staticmethod
    def _marks_kept(marks):
        return {"fresh maps kept": int(marks[0] == marks[1]), "lazy maps kept": int(marks[2] == marks[3])}

    def do_split_clouds(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        n = len(op["slots"])
        words = {"points": 4, "height": 1, "source": 1}
        with self.on(op["stream"]):
            x = _lib.GGCloudSplit()
            n_pts, stride, keep = self._cloud_source(op, x)
            bufs = {(s, f): self._words(n * stride * words[f]) for s, fields in op["want"].items() for f in fields}
            counts = self._words(n * 2)
            for (s, f), t in bufs.items():
                setattr(getattr(x, s), "d_" + f, t.data_ptr())
            x.d_counts = counts.data_ptr()
            marks = self._enqueue(op, lambda st: self.seg._L.gg_split_clouds(self.seg._ctx, C.byref(x), st))
        self.keep.append((bufs, counts))

        def collect():
            res = self._marks_kept(marks)
            c = counts.cpu().numpy()
            clean = bool(np.all(c[n * 2:] == SENTINEL))
            host = {key: t.cpu().numpy() for key, t in bufs.items()}
            for i, s in enumerate(op["slots"]):
                for col, name in enumerate(("ground", "nonground")):
                    m = int(c[2 * i + col])
                    res[f"cloud {i} (slot {s}) {name} count"] = np.int32(m)
                    m = min(max(m, 0), stride)
                    for f in op["want"].get(name, []):
                        w = words[f]
                        row = host[(name, f)][i * stride * w: (i + 1) * stride * w]
                        clean &= bool(np.all(row[m * w:] == SENTINEL))
                        got = row[: m * w]
                        res[f"cloud {i} (slot {s}) {name} {f}"] = got.view(np.uint32).reshape(-1, 4) if f == "points" else got.view(np.float32) if f == "height" else got
            for key, a in host.items():
                clean &= bool(np.all(a[n * stride * words[key[1]]:] == SENTINEL))
            res["nothing else written"] = int(clean)
            return res

        return collect

    def do_rasterize_clouds(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        n, K, pstride = len(op["slots"]), len(op["channels"]), self.seg.rows * self.seg.cols + int(op["pad"])
        with self.on(op["stream"]):
            x = _lib.GGCloudRaster()
            n_pts, stride, keep = self._cloud_source(op, x)
            dst = self._words(n * K * pstride)
            x.channel_mask = sum(1 << RASTER_CHANNELS.index(k) for k in op["channels"])
            x.order = _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR
            x.d_dst, x.plane_stride = dst.data_ptr(), pstride
            marks = self._enqueue(op, lambda st: self.seg._L.gg_rasterize_clouds(self.seg._ctx, C.byref(x), st))
        self.keep.append(dst)

        def collect():
            res = self._marks_kept(marks)
            planes, clean = self._planes(dst.cpu().numpy(), n, K, pstride, op["row_major"])
            for i, s in enumerate(op["slots"]):
                for k, name in enumerate(op["channels"]):
                    res[f"cloud {i} (slot {s}) {name}"] = planes[i * K + k].view(np.uint32)
            res["nothing else written"] = int(clean)
            return res

        return collect

    @staticmethod
    def _set_band(x, op):
        x.min_points = op["min_points"]
        x.min_height = -np.inf if op["min_height"] is None else op["min_height"]
        x.max_height = np.inf if op["max_height"] is None else op["max_height"]

    def do_cluster_clouds(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        n, pstride, cap = len(op["slots"]), self.seg.rows * self.seg.cols + int(op["pad"]), op["max_clusters"]
        with self.on(op["stream"]):
            x = _lib.GGCloudClusters()
            n_pts, stride, keep = self._cloud_source(op, x)
            self._set_band(x, op)
            planes, count = self._words(n * pstride), self._words(n)
            table = self._words(n * cap * 8) if cap else None
            ids = self._words(n * stride) if op["point_clusters"] else None
            x.connectivity, x.order = op["connectivity"], _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR
            x.d_cell_cluster, x.plane_stride, x.d_n_clusters = planes.data_ptr(), pstride, count.data_ptr()
            x.d_point_cluster = ids.data_ptr() if ids is not None else None
            x.d_clusters, x.max_clusters = (table.data_ptr() if cap else None), cap
            marks = self._enqueue(op, lambda st: self.seg._L.gg_cluster_clouds(self.seg._ctx, C.byref(x), st))
        self.keep.append((planes, count, table, ids))
        self.dev_outs[self.at] = {"cell ids": (planes, pstride, n, op["row_major"]), "clusters": (count, 1, n, op["row_major"]), "_points": self.last_points}
        if ids is not None:
            self.dev_outs[self.at]["point ids"] = (ids, stride, n, op["row_major"])

        def collect():
            res = self._marks_kept(marks)
            cells, clean = self._planes(planes.cpu().numpy(), n, 1, pstride, op["row_major"])
            c = count.cpu().numpy()
            clean &= bool(np.all(c[n:] == SENTINEL))
            t = table.cpu().numpy() if cap else None
            p = ids.cpu().numpy() if ids is not None else None
            for i, s in enumerate(op["slots"]):
                res[f"cloud {i} (slot {s}) cell ids"] = cells[i]
                res[f"cloud {i} (slot {s}) clusters"] = np.int32(c[i])
                if cap:
                    m = min(max(int(c[i]), 0), cap)
                    rec = t[i * cap * 8: (i + 1) * cap * 8]
                    res[f"cloud {i} (slot {s}) table"] = rec[: m * 8].view(np.uint32).reshape(-1, 8)
                    clean &= bool(np.all(rec[m * 8:] == SENTINEL))
                if p is not None:
                    row = p[i * stride: (i + 1) * stride]
                    res[f"cloud {i} (slot {s}) point ids"] = row[: n_pts[i]]
                    clean &= bool(np.all(row[n_pts[i]:] == SENTINEL))
            if cap:
                clean &= bool(np.all(t[n * cap * 8:] == SENTINEL))
            if p is not None:
                clean &= bool(np.all(p[n * stride:] == SENTINEL))
            res["nothing else written"] = int(clean)
            return res

        return collect

    def do_clearance_clouds(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        n, pstride = len(op["slots"]), self.seg.rows * self.seg.cols + int(op["pad"])
        with self.on(op["stream"]):
            x = _lib.GGCloudClearance()
            n_pts, stride, keep = self._cloud_source(op, x)
            self._set_band(x, op)
            dist2, count = self._words(n * pstride), self._words(n)
            nearest = self._words(n * pstride) if op["nearest"] else None
            distance = self._words(n * pstride) if op["distance"] else None
            x.max_cells, x.order = op["max_cells"], _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR
            x.d_dist2, x.plane_stride, x.d_n_occupied = dist2.data_ptr(), pstride, count.data_ptr()
            x.d_nearest = nearest.data_ptr() if nearest is not None else None
            x.d_distance = distance.data_ptr() if distance is not None else None
            marks = self._enqueue(op, lambda st: self.seg._L.gg_clearance_clouds(self.seg._ctx, C.byref(x), st))
        self.keep.append((dist2, count, nearest, distance))
        self.dev_outs[self.at] = {"dist2": (dist2, pstride, n, op["row_major"])}

        def collect():
            res = self._marks_kept(marks)
            c = count.cpu().numpy()
            clean = bool(np.all(c[n:] == SENTINEL))
            got = {}
            for name, t in (("dist2", dist2), ("nearest", nearest), ("distance bits", distance)):
                if t is not None:
                    got[name], ok = self._planes(t.cpu().numpy(), n, 1, pstride, op["row_major"])
                    clean &= ok
            for i, s in enumerate(op["slots"]):
                for name, planes in got.items():
                    res[f"cloud {i} (slot {s}) {name}"] = planes[i].view(np.uint32) if name == "distance bits" else planes[i]
                res[f"cloud {i} (slot {s}) occupied cells"] = np.int32(c[i])
            res["nothing else written"] = int(clean)
            return res

        return collect

    def do_visibility_clouds(self, op):
        import ctypes as C

        from groundgrid_amd import _lib

        n, pstride = len(op["slots"]), self.seg.rows * self.seg.cols + int(op["pad"])
        with self.on(op["stream"]):
            x = _lib.GGCloudVisibility()
            n_pts, stride, keep = self._cloud_source(op, x)
            self._set_band(x, op)
            state = self._words(n * pstride)
            counts = self._words(n * 3) if op["counts"] else None
            origins = np.ascontiguousarray(np.asarray(op["origins"], dtype=np.float32).reshape(n, 3))
            x.origins = origins.ctypes.data_as(C.POINTER(C.c_float))
            x.max_cells, x.order = op["max_cells"], _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR
            x.d_state, x.plane_stride = state.data_ptr(), pstride
            x.d_counts = counts.data_ptr() if counts is not None else None
            marks = self._enqueue(op, lambda st: self.seg._L.gg_visibility_clouds(self.seg._ctx, C.byref(x), st))
        self.keep.append((state, counts))
        self.dev_outs[self.at] = {"state": (state, pstride, n, op["row_major"])}

        def collect():
            res = self._marks_kept(marks)
            planes, clean = self._planes(state.cpu().numpy(), n, 1, pstride, op["row_major"])
            c = counts.cpu().numpy() if counts is not None else None
            for i, s in enumerate(op["slots"]):
                res[f"cloud {i} (slot {s}) state"] = planes[i]
                if c is not None:
                    res[f"cloud {i} (slot {s}) counts"] = c[3 * i: 3 * i + 3]
            if c is not None:
                clean &= bool(np.all(c[3 * n:] == SENTINEL))
            res["nothing else written"] = int(clean)
            return res

        return collect

    def state(self, s, with_scores):
        """what ContextModel.state(s) describes, read through the getters"""
        out = {f"layer {k}": v for k, v in self.seg.map(s).layers().items()}
        out["position"] = self.library_position(s)
        assert np.array_equal(out["position"], self.do_get_position(dict(slot=s))["position"]), f"slot {s}: GridMap.getPosition is stale"
        out.update(self.do_slot_config(dict(slot=s)))
        if with_scores:
            clouds, counts = self.seg.scores_raw(slots=[s])
            out["score clouds"], out["score counts"] = np.uint64(clouds[0]), counts[0]
        return out

    def release(self):
        for planes in self.planes.values():
            self.seg.release_layers(planes)
        self.planes = {}


for _kind in PLANE_KINDS:
    setattr(Driver, "do_" + _kind, lambda self, op: seq_planes.device_op(self, op))
for _kind in LATE_KINDS:
    setattr(Driver, "do_" + _kind, lambda self, op: seq_late.device_op(self, op))


class _NoContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def run_on_device(seg, ops, shape, on_result=None):
    """Issue `ops` on the context `seg`; returns the Driver (for the final state)."""
    d = Driver(seg, shape, on_result)
    d.run(ops)
    return d
