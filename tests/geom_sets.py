"""The two sensor constants of gg_create (gg_geometry.vertical_point_ang_dist / min_dist_squared: compile-time constants of
include/groundgrid/GroundSegmentation.h:69-70 in the reference) moved off their defaults: the constant sets, and the scenes that use them.
A plain helper module shared by tests/test_geometry_constants_cpu.py (sensitivity, on the oracle alone), tests/test_geometry_constants_gpu.py,
the two sweep emulator files, tests/test_oracle_cpu.py and tests/ref_scenes.py.  Nothing here reads the reference.

min_dist_squared reaches the device twice: as a float in the ignore test (:237, `sqdist < min`, strict) and as the integer threshold
r2min of the confidence decay (:463, `(dx^2 + dy^2) * resolution^2 > min`, strict, restated as dx^2 + dy^2 >= r2min with a different index
expression at every place a sweep visits a cell).  Each set is chosen by WHERE it puts r2min; r2min() below is the same formula the host
uses, and check_class() asserts that a set's number lands in the class it is named for.

  set  geometry      min_dist_squared          r2min     class
  A    120 / 0.33    446.0                     4096      = 64^2: the on-axis cell of ring 64, the last ring of the first 64-ring group,
                                                         is the first to decay; vertical_point_ang_dist = 0.00174532925 (0.1 degrees)
  B    61 / 0.25     264.0625 = 4225 / 16      4226      resolution^2 = 1/16 is exact: r^2 = 4225 = 65^2 = 16^2 + 63^2 = 25^2 + 60^2 =
                                                         33^2 + 56^2 = 39^2 + 52^2 sits EXACTLY on the strict boundary (no decay), 4226
                                                         = 65^2 + 1 decays; vertical_point_ang_dist = twice the default
  C    61 / 0.25     (21557 - 0.5) / 16        21557     between c^2 = 14641 and 2 (c - 1)^2 = 28800 (c = 121): no on-axis cell decays,
                                                         only the corner triangles of the outer rings (21556 and 21557 are both sums
                                                         of two squares of the map: either neighbour of the threshold moves cells)
  D    33 / 0.33     66^2 = 4356               2 n^2     larger than the whole diagonal squared: nothing decays, every in-map point is
                                                         GG_CLASS_IGNORED (the returned cloud is the ignored block alone)
  E    120 / 0.33    0.01                      1         everything but the centre decays, nothing is ignored by distance
  F    43 / 0.33     default                   111       vertical_point_ang_dist = 1e-8: floor(threshold * S * expected) >= 2^24 within
                                                         ~4 cells of the centre (the INFINITY branch of the patch table), huge elsewhere
"""
from __future__ import annotations

import functools

import numpy as np

from groundgrid_amd import synth
from tests import edge_scenes as es

DEFAULT_VPAD = float(np.float32(0.00174532925 * 2))   # what zero selects
DEFAULT_MDS = 12.0

SETS = {
    #      length  resolution  vertical_point_ang_dist                  min_dist_squared           class
    "A": (120.0, 0.33, float(np.float32(0.00174532925)), 446.0, "group_boundary"),
    "B": (61.0, 0.25, float(np.float32(0.00174532925 * 4)), 264.0625, "strict_boundary"),
    "C": (61.0, 0.25, 0.0, (21557 - 0.5) / 16.0, "corners_only"),
    "D": (33.0, 0.33, 0.0, 4356.0, "nothing_decays"),
    "E": (120.0, 0.33, 0.0, 0.01, "everything_decays"),
    "F": (43.0, 0.33, 1e-8, 0.0, "absurd_table"),
}
R2MIN_SETS = "ABCDE"   # the sets that move min_dist_squared


def cells(length, resolution) -> int:
    """grid_map::GridMap::setGeometry: round(length / resolution) on the float constants"""
    return int(round(float(np.float32(length)) / float(np.float32(resolution))))


def r2min(n, resolution, min_dist_squared) -> int:
    """the smallest integer r2 with r2 * resolution^2 > min_dist_squared in double on the float constants (:463), capped at 2 n^2: the
    formula of gg::sweep::make_params, restated"""
    res = float(np.float32(resolution))
    mds = float(np.float32(min_dist_squared if min_dist_squared else DEFAULT_MDS))
    r2 = 0
    while r2 < 2 * n * n and not (r2 * (res * res) > mds):
        r2 += 1
    return r2


def min_dist_sq_for(cls, n, resolution) -> float:
    """a min_dist_squared that puts r2min of ANY n x n map into class C, D or E (the emulator files sweep many geometries)"""
    res = float(np.float32(resolution))
    c = n // 2 - 1
    if cls == "corners_only":
        t = (c * c + 2 * (c - 1) * (c - 1)) // 2
        return float(np.float32((t - 0.5) * res * res))
    if cls == "nothing_decays":
        return float(np.float32(2.0 * (n * res) * (n * res)))
    if cls == "everything_decays":
        return float(np.float32(0.5 * res * res))
    raise ValueError(cls)


def check_class(cls, n, r2) -> None:
    """r2 lies where the class says (c = n / 2 - 1 is the sweep's centre, rings 1 .. c - 1 are swept, a cell of ring r has r^2 <= dx^2 + dy^2 <= 2 r^2)"""
    c = n // 2 - 1
    if cls == "group_boundary":
        assert r2 in (64 * 64, 65 * 65) and c - 1 > 65, (r2, c)
    elif cls == "strict_boundary":
        assert r2 == 4226 and 65 < c - 1, (r2, c)
    elif cls == "corners_only":
        assert c * c < r2 < 2 * (c - 1) * (c - 1), (r2, c)
    elif cls == "nothing_decays":
        assert r2 == 2 * n * n and r2 > 2 * c * c, (r2, n)
    elif cls == "everything_decays":
        assert r2 == 1, r2
    elif cls == "absurd_table":
        assert r2 == r2min(n, 0.33, DEFAULT_MDS), r2
    else:
        raise ValueError(cls)


def geometry(name):
    """(length, resolution, vertical_point_ang_dist, min_dist_squared) of a set, as gg_geometry takes them (0 = the reference's value)"""
    return SETS[name][:4]


def oracle_map(name, **kw):
    from oracle import oracle

    L, R, vpad, mds, _ = SETS[name]
    return oracle.OracleMap(L, R, vertical_point_ang_dist=vpad, min_dist_squared=mds, **kw)


# ---------------------------------------------------------------- the sweep emulators' cases
# (tag, length, resolution): a constant set on its own geometry, or a class on any geometry (one, two and three 64-ring groups)
R2MIN_CASES = [("A", 120.0, 0.33), ("B", 61.0, 0.25)] + [(cls, L, R) for cls in ("corners_only", "nothing_decays", "everything_decays")
                                                        for L, R in ((33.0, 0.33), (61.0, 0.25), (120.0, 0.33))]


def r2min_case(tag, length, resolution):
    """(min_dist_squared, r2min, oracle map created with that constant); asserts that r2min lies in the class the case is named for"""
    n = cells(length, resolution)
    if tag in SETS:
        L, R, _, mds, cls = SETS[tag]
        assert (L, R) == (length, resolution)
    else:
        mds, cls = min_dist_sq_for(tag, n, resolution), tag
    r2 = r2min(n, resolution, mds)
    check_class(cls, n, r2)
    from oracle import oracle

    ref = oracle.OracleMap(length, resolution, min_dist_squared=mds)
    assert ref.rows == n and np.float32(ref.min_dist_squared) == np.float32(mds)
    return mds, r2, ref



# ---------------------------------------------------------------- scenes: >= 4 frames on one map, the cloud SHRINKING from frame to frame
# (clouds in firing order, one azimuth column after the other: a shorter prefix drops a whole sector of bearings, near and far points alike, so
# the cells of that sector lose their observations and only the decay moves their confidence.  A ring-major cloud would not do: its tail
# is the near rings, which sets A and B ignore anyway, and no cell would lose anything.)
FRAMES = 4
# the point the ignore test (:237) measures from.  Sets B and C ignore 264 m^2 and 1347 m^2 around it on a 61 m map: measured from the map's
# centre that leaves a few hundred kept points (B) or none (C).  Off the centre both classes are there in their thousands in every frame
# (B: the disc lies in the sector the shrinking cloud keeps longest; C: over the map's corner), and set B's cells on both sides of its decay
# boundary, 16.25 m around the CENTRE, are observed
ORIGINS = {"B": (-14.0, 10.0, 0.1), "C": (35.0, 30.0, 0.3)}


def frame_points(n, frame) -> int:
    """how many points of an n-point cloud frame `frame` uses: all, then 15 % fewer per frame"""
    return n - (n * 15 * frame) // 100


def scaled_cloud(length, seed, n_az, angle=0.0) -> np.ndarray:
    """a sensor cloud scaled to cover a map of `length` metres, rotated by `angle`"""
    base = synth.hdl64_cloud(seed=seed, n_az=n_az, order="azimuth")
    c = synth.clone_cloud(base)
    k = np.float32(length / 120.0)
    a = np.float32(angle)
    c["x"] = ((np.cos(a) * base["x"] - np.sin(a) * base["y"]) * k).astype(np.float32)
    c["y"] = ((np.sin(a) * base["x"] + np.cos(a) * base["y"]) * k).astype(np.float32)
    return c


# the batched launch shapes of tests/test_geometry_constants_gpu.py: clouds per call.  17 .. 64: k_sweep in parts; > 256 fresh maps:
# k_sweep<FRESH>, plain and as two concurrent halves; the throughput pair sweep is forced (tuning sweep_pair = 4) on a small batch
BATCH_COUNTS = {"parts": 24, "fresh": 257, "halves": 260, "throughput": 3}
BATCH_BASE_Z = -1.73


def batch_clouds(name, count, n_az=120, seed=61):
    """cloud b of every batch of a set: the same sensor cloud turned by 0.31 b (a shorter batch is a prefix of a longer one)"""
    base = synth.hdl64_cloud(seed=seed, n_az=n_az, order="azimuth")
    k = np.float32(SETS[name][0] / 120.0)
    out = []
    for b in range(count):
        c = synth.clone_cloud(base)
        a = np.float32(0.31 * b)
        c["x"] = ((np.cos(a) * base["x"] - np.sin(a) * base["y"]) * k).astype(np.float32)
        c["y"] = ((np.sin(a) * base["x"] + np.cos(a) * base["y"]) * k).astype(np.float32)
        out.append(c)
    return out


def batch_origin(name):
    return ORIGINS.get(name, (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def scene(name) -> es.Scene:
    """the single-map scene of a set: FRAMES frames of one shrinking cloud; extra carries the constants and the per-frame point counts"""
    L, R, vpad, mds, cls = SETS[name]
    cloud = scaled_cloud(L, 40 + ord(name), 700 if L > 100 else 500)
    return es.Scene("geom/" + name, cloud, f"gg_geometry constants off their defaults: {cls}", length=L, resolution=R,
                    origin=ORIGINS.get(name, (0.25, -0.125, 0.1)), base_z=-1.73, frames=FRAMES,
                    extra={"vertical_point_ang_dist": vpad, "min_dist_squared": mds,
                           "frame_points": [frame_points(len(cloud), f) for f in range(FRAMES)]})


def frame_cloud(sc, frame) -> np.ndarray:
    """the cloud of frame `frame` of a scene (the whole cloud unless the scene shrinks it)"""
    fp = sc.extra.get("frame_points")
    return sc.cloud if fp is None else sc.cloud[: fp[frame]]


def scene_constants(sc):
    return float(sc.extra.get("vertical_point_ang_dist", 0.0)), float(sc.extra.get("min_dist_squared", 0.0))


# ---------------------------------------------------------------- clouds for the ignore test (:237, strict <, on a float rounded from double)
def sqdist_f32(dx, dy) -> np.float32:
    """:223 as the reference computes it: float products promoted to double, the sum rounded to float"""
    dx, dy = np.float32(dx), np.float32(dy)
    return np.float32(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy))


def _points_with_sqdist(target, count, rng):
    """`count` float pairs (dx, dy), in all four quadrants, whose :223 is EXACTLY the float `target`: dy a dyadic fraction that carries most of
    the sum, dx the rounded root of the rest (its rounding error is far below half an ulp of the sum), verified and searched a few ulps around"""
    target = np.float32(target)
    out = []
    root = float(np.sqrt(np.float64(target)))
    tries = 0
    while len(out) < count:
        tries += 1
        assert tries < 10000, f"no float pair with sqdist {target!r}"
        frac = rng.uniform(0.3, 0.999)
        dy = np.float32(np.round(root * frac * 64.0) / 64.0)
        rest = np.float64(target) - np.float64(dy) * np.float64(dy)
        if rest <= 0:
            continue
        dx0 = np.float32(np.sqrt(rest))
        for k in range(-3, 4):
            dx = dx0
            for _ in range(abs(k)):
                dx = np.nextafter(dx, np.float32(np.inf if k > 0 else -np.inf))
            if sqdist_f32(dx, dy) == target:
                sx, sy = rng.choice([-1.0, 1.0], 2)
                pair = (np.float32(sx) * dx, np.float32(sy) * dy) if len(out) % 2 else (np.float32(sy) * dy, np.float32(sx) * dx)
                out.append(pair)
                break
    return out


def exact_pairs(name):
    """set B only: the dyadic points whose :223 is 264.0625 with no rounding anywhere (quarters of 65^2 = 16^2 + 63^2 = ...), all sign and axis choices"""
    assert name == "B"
    out = []
    for a, b in ((65, 0), (16, 63), (25, 60), (33, 56), (39, 52)):
        for sa in (-1, 1):
            for sb in (-1, 1):
                out += [(np.float32(sa * a / 4.0), np.float32(sb * b / 4.0)), (np.float32(sb * b / 4.0), np.float32(sa * a / 4.0))]
    return out


IGNORE_SETS = ["A", "B", "E", "default"]   # (C: the ignore radius lies outside the map from most origins; D: every in-map point is inside it)


@functools.lru_cache(maxsize=None)
def ignore_cloud(name):
    """(cloud, origin, special, length, resolution, vpad, mds): a sensor cloud with points whose :223 is exactly min_dist_squared, the float
    below it and the float above it -- `special` = {"at" | "below" | "above": indices} -- spread over the whole cloud (one every ~60 points:
    different wavefronts and chunks; different bearings: different tiles).  The origin is (0, 0, .) so that dx = x exactly."""
    L, R, vpad, mds, _ = SETS[name] if name != "default" else (120.0, 0.33, 0.0, 0.0, "")
    m = np.float32(mds if mds else DEFAULT_MDS)
    rng = np.random.default_rng(500 + sum(name.encode()))
    base = scaled_cloud(L, 7, 180)
    targets = {"at": m, "below": np.nextafter(m, np.float32(-np.inf)), "above": np.nextafter(m, np.float32(np.inf))}
    pairs = []
    for kind, t in targets.items():
        pairs += [(kind, p) for p in _points_with_sqdist(t, 24, rng)]
    if name == "B":
        pairs += [("at", p) for p in exact_pairs("B")]
    order = rng.permutation(len(pairs))
    stride = max(len(base) // len(pairs), 1)
    cloud = synth.clone_cloud(base)
    special = {"at": [], "below": [], "above": []}
    for k, o in enumerate(order):
        kind, (dx, dy) = pairs[o]
        i = k * stride + int(rng.integers(0, stride))
        cloud["x"][i], cloud["y"][i], cloud["z"][i] = dx, dy, np.float32(-1.7)
        cloud["ring"][i] = k % 64
        special[kind].append(i)
    half = 0.5 * cells(L, R) * float(np.float32(R))
    for kind, t in targets.items():
        idx = np.array(special[kind])
        assert (np.abs(cloud["x"][idx]) < half - 1).all() and (np.abs(cloud["y"][idx]) < half - 1).all(), "a boundary point left the map"
        got = np.array([sqdist_f32(cloud["x"][i], cloud["y"][i]) for i in idx])
        assert (got == t).all(), (name, kind)
    return cloud, (0.0, 0.0, 0.2), {k: np.array(sorted(v)) for k, v in special.items()}, L, R, vpad, mds
