"""Seeded hostile scenes shared by the single-cloud parity tests (tests/test_gpu_parity.py), the batched parity tests
(tests/test_gpu_batch_edges.py) and the CPU guard that checks every scene still reaches the branch it is named for
(tests/test_edge_scenes_cpu.py).  A plain helper module: the product never imports it.

Every generator returns a Scene: the cloud (map frame, PointXYZIR) and what the scene needs to run -- geometry, map position,
sensor origin, base height, initial height, a configuration edit, the frame count -- plus `branch`, a line naming the path of
the device code it is meant to reach.  The inputs of the single-cloud scenes are exactly those the tests built inline before.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from groundgrid_amd import synth
from oracle import oracle

ORIGIN0 = (0.0, 0.0, 0.0)
RCAP = 4080        # k_reduce's reciprocal table: a cell with more points takes the IEEE tail
K2_LIGHT_MAX = 512  # tiles with at most this many records are reduced by one wavefront, larger ones by a work-group
TILE = 16


@dataclass
class Scene:
    name: str
    cloud: np.ndarray
    branch: str
    length: float = 120.0
    resolution: float = 0.33
    pos: tuple = (0.0, 0.0)
    origin: tuple = ORIGIN0
    base_z: float = -1.73
    odom_z: float = 0.0
    frames: int = 2
    cfg_edit: Optional[Callable] = None
    extra: dict = field(default_factory=dict)


# ---------------------------------------------------------------- the single-cloud scenes, as the parity tests build them

def edge_cases() -> Scene:
    """NaN and +-inf in x, y and z, ring 2000 (above max_ring), points on the map border, -1e30, a point 500 m out."""
    pts = np.array([[5, 5, -1], [1, 1, -1], [5, 5, -1], [500, 0, -1], [np.nan, 0, -1], [5, 5, np.nan], [-59.9, -59.9, -1],
                    [np.inf, 1, 0], [59.99, 59.99, 0.5], [0, 0, 3], [3, -59.5, -1.6], [5, 5, -np.inf], [-1e30, 2, 0]],
                   dtype=np.float32)
    cloud = synth.make_cloud(pts, ring=[0, 0, 2000, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5])
    return Scene("edge_cases", cloud, "k_classify: non-finite coordinates outside, ring > max_ring IGNORED; k_reduce: NaN / -inf heights")


def signalling_nan_heights() -> Scene:
    """A SIGNALLING NaN height between two ordinary returns of one cell (np.nan is a quiet one): std::max(mx, z) of :307 must
    leave the cell's maximum alone (k2_reduce.hip quiet)."""
    snan = synth.make_cloud(np.array([[5, 5, -1.2], [5.01, 5.01, 0.0], [5.02, 5.0, -1.1], [7, 7, 0.0], [7.01, 7.0, -1.0]], dtype=np.float32))
    z = snan["z"].view(np.uint32)
    z[1] = 0x7FA00000
    z[3] = 0xFF800001
    return Scene("signalling_nan_heights", snan, "k_reduce: the maximum of a cell with signalling-NaN heights (quiet)")


def empty() -> Scene:
    return Scene("empty", synth.empty_cloud(0), "every kernel on a cloud without points")


def all_outside() -> Scene:
    return Scene("all_outside", synth.make_cloud(np.array([[900.0, 900.0, 0.0]], dtype=np.float32)), "k_classify: no point inside the map",
                 frames=1)


def dense_single_cells_and_ties() -> Scene:
    """thousands of points in a handful of cells: long ordered Welford chains, LDS staging over several chunks"""
    rng = np.random.default_rng(4)
    n = 30000
    xy = rng.choice(np.array([5.0, 5.2, 5.4, 7.7]), size=(n, 2)) + rng.uniform(0, 0.05, size=(n, 2))
    z = rng.normal(-1.7, 0.05, size=n)
    return Scene("dense_single_cells_and_ties", synth.make_cloud(np.column_stack([xy, z]), ring=rng.integers(0, 64, n)),
                 "k_reduce: dense tiles, cells with thousands of points (more than RCAP)")


def reduce_tile_classes_long_cells_and_quotient_fallbacks() -> Scene:
    """k_reduce's corner cases: a cell with more points than the reciprocal table holds (IEEE tail), constant heights (every
    delta is 0: all quotients take the exact path), heights so small that quotients fall below 2^-100, huge heights, and two
    regions of 512 / 513 points meant for the single-wavefront / work-group tile paths (their regions straddle a tile border: the
    exact counts are in exact_tile_records())."""
    rng = np.random.default_rng(77)
    res = 0.33
    parts = []

    def cell_points(cx, cy, n, z):
        xy = np.column_stack([np.full(n, cx), np.full(n, cy)]) + rng.uniform(0.01, res - 0.01, size=(n, 2))
        return np.column_stack([xy, z])

    # one cell with 5000 points (> RCAP = 4080), noisy heights
    parts.append(cell_points(6 * res, 6 * res, 5000, rng.normal(-1.7, 0.03, 5000)))
    # one cell, constant height: mean == planeDist from the second point on
    parts.append(cell_points(-9 * res, 4 * res, 700, np.full(700, -1.5, np.float32)))
    # tiny and huge heights
    parts.append(cell_points(12 * res, -7 * res, 300, rng.normal(0, 1, 300) * 1e-36))
    parts.append(cell_points(-14 * res, -11 * res, 300, rng.normal(0, 1, 300) * 1e30))
    # 512 and 513 points spread over about one tile of 16x16 cells
    for tile_x, count in ((40, 512), (60, 513)):
        xy = np.column_stack([rng.uniform(tile_x * res + 0.02, (tile_x + 15) * res, count), rng.uniform(-90 * res, -76 * res, count)])
        parts.append(np.column_stack([xy, rng.normal(-1.7, 0.05, count)]))
    pts = np.concatenate(parts).astype(np.float32)
    rng.shuffle(pts)
    return Scene("reduce_tile_classes", synth.make_cloud(pts, ring=rng.integers(0, 64, len(pts))),
                 "k_reduce: a cell over RCAP, exact-zero deltas, tiny / huge quotients")


def _tile_centre_range(length, res, tile_index):
    """map-frame coordinate range (lo, hi) of the cells of tile row (or column) `tile_index` of a map at (0, 0): cell k covers
    (L/2 - (k + 1) res, L/2 - k res], its interior shrunk by 0.02 m so that no point sits near a boundary"""
    n = int(round(length / res))
    L = n * np.float64(np.float32(res))
    k0, k1 = tile_index * TILE, tile_index * TILE + TILE - 1
    return L / 2 - (k1 + 1) * np.float64(np.float32(res)) + 0.02, L / 2 - k0 * np.float64(np.float32(res)) - 0.02


def exact_tile_records() -> Scene:
    """Tiles holding EXACTLY 511, 512 (the largest the single-wavefront path takes), 513 (the smallest of the work-group path) and
    1024 records, each spread over the cells of one 16x16 tile, and a cell of 4081 points (one more than the reciprocal table)
    alone in its tile."""
    rng = np.random.default_rng(5120)
    parts = []
    for (tr, tc), count in (((3, 3), 511), ((3, 8), 512), ((8, 3), 513), ((8, 8), 1024)):
        xlo, xhi = _tile_centre_range(120.0, 0.33, tr)
        ylo, yhi = _tile_centre_range(120.0, 0.33, tc)
        xy = np.column_stack([rng.uniform(xlo, xhi, count), rng.uniform(ylo, yhi, count)])
        parts.append(np.column_stack([xy, rng.normal(-1.7, 0.05, count)]))
    res = np.float64(np.float32(0.33))
    cx = 0.5 * 364 * res - (14 * TILE + 5.5) * res  # the centre of cell (229, 229)
    parts.append(np.column_stack([cx + rng.uniform(-0.1, 0.1, (RCAP + 1, 2)), rng.normal(-1.6, 0.02, RCAP + 1)]))
    pts = np.concatenate(parts).astype(np.float32)
    rng.shuffle(pts)
    return Scene("exact_tile_records", synth.make_cloud(pts, ring=rng.integers(0, 64, len(pts))),
                 "k_reduce: tiles of exactly 512 (wavefront) and 513 (work-group) records, a cell of RCAP + 1 points",
                 extra={"tile_records": {511: 1, 512: 1, 513: 1, 1024: 1}})


RECURRENCE_SEQS_FIXED = [
    [0.0, 0.0, 0.5, -0.5, 0.25, 0.0, 1.0],
    [1.0, -1.0, 3.0, 0.125, -0.125],          # the mean returns to exactly 0 after the second point
    [-0.0, 2.0, -2.0, -0.0, 0.0, 7.0],
    [2.0, 2.0, -4.0, 1.0, 1.0, 1.0, 1.0, -4.0],
    [-1.7, np.inf, -1.6, -np.inf, -1.5, -1.4],
]


def reduce_recurrence_rare_cases() -> Scene:
    """k_reduce's fast recurrence assumes `mean != 0` after a cell's first point and heights that are numbers; four points
    that break either are redone with the reference's expressions.  Cells whose running mean is or returns to exactly zero,
    NaN / +-inf heights at every position of a four-point block, -0.0, in a light tile (one wavefront), in a dense tile
    (work-group, count-sorted lanes) and in a tile whose fullest cells run one chain per wavefront."""
    rng = np.random.default_rng(123)
    res = 0.33
    seqs = [list(s) for s in RECURRENCE_SEQS_FIXED]
    for k in range(9):                               # a NaN at position k
        z = list(rng.normal(-1.7, 0.02, 12))
        z[k] = np.nan
        seqs.append(z)
    long_cell = list(rng.normal(-1.7, 0.02, 40))    # >= 24 points: the tile's fullest cells run one chain per wavefront
    long_cell[17] = 0.0
    long_cell[23] = np.nan
    long_cell[24] = 0.0
    long_cell[25] = 0.0
    seqs.append(long_cell)

    def region(x0, y0, fillers):
        """the sequences in cells (x0 + k, y0) ... of one 16x16 tile, `fillers` more points spread over the tile's other rows"""
        parts = []
        for k, z in enumerate(seqs):
            cx, cy = (x0 + k % 16) * res, (y0 + k // 16) * res
            xy = np.column_stack([np.full(len(z), cx), np.full(len(z), cy)]) + rng.uniform(0.02, res - 0.02, size=(len(z), 2))
            parts.append(np.column_stack([xy, np.asarray(z, np.float64)]))
        if fillers:
            xy = np.column_stack([rng.uniform(x0 * res + 0.02, (x0 + 15) * res, fillers), rng.uniform((y0 + 3) * res, (y0 + 12) * res, fillers)])
            parts.append(np.column_stack([xy, rng.normal(-1.7, 0.05, fillers)]))
        return np.concatenate(parts)

    # (a region straddles up to four tiles: enough fillers that its tiles leave the single-wavefront path / split their chains)
    pts = np.concatenate([region(30, 30, 0), region(-70, 30, 3000), region(30, -70, 12000)]).astype(np.float32)
    return Scene("reduce_recurrence_rare_cases", synth.make_cloud(pts, ring=rng.integers(0, 64, len(pts))),
                 "k_reduce: zero means, NaN / +-inf / -0.0 heights off the fast recurrence")


def line_of_sight_clouds():
    """(base, low): a sensor cloud and the same with one point in five 0.3 .. 2.5 m under the surface (outlier candidates for
    the line-of-sight walk of k_classify)"""
    base = synth.hdl64_cloud(seed=12, n_az=900)
    rng = np.random.default_rng(12)
    low = synth.clone_cloud(base)
    sel = rng.random(len(low)) < 0.2            # one point in five dives 0.3 .. 2.5 m under the surface
    low["z"][sel] -= rng.uniform(0.3, 2.5, sel.sum()).astype(np.float32)
    return base, low


LINE_OF_SIGHT_ORIGINS = [ORIGIN0, ORIGIN0, (7.5, -3.0, 0.4), (-80.0, 20.0, 1.0)]


def line_of_sight_walk() -> Scene:
    """the low cloud seen from off the map centre: from the second frame on (warm map) the walk marks OUTLIERs"""
    _, low = line_of_sight_clouds()
    return Scene("line_of_sight_walk", low, "k_classify: the cooperative line-of-sight walk (OUTLIER)", origin=(7.5, -3.0, 0.4), frames=2)


def corrupt_z_cloud() -> np.ndarray:
    good = synth.hdl64_cloud(seed=2, n_az=300)
    bad = synth.make_cloud(np.array([[4.0, 4.0, -1e9], [10.0, -3.0, -3e38], [0.2, 25.0, -1e7], [7.0, 7.0, -70000.0]], dtype=np.float32))
    cloud = synth.empty_cloud(len(good) + len(bad))
    cloud[: len(good)] = good
    cloud[len(good):] = bad
    return cloud


def corrupt_z() -> Scene:
    """in-map points with z = -1e9 .. -3e38: the bounded line-of-sight walk (documented deviation shared with the oracle)"""
    return Scene("corrupt_z", corrupt_z_cloud(), "k_classify: the bounded line-of-sight walk", frames=3)


def index_fast_path_boundaries() -> Scene:
    """points exactly on / next to cell boundaries: K1's multiply + exactness check of getIndex must decide like the divide"""
    m = oracle.OracleMap(120.0, 0.33)
    half, res = 0.5 * m.length[0], m.resolution
    xs = []
    for k in (0, 1, 2, 17, 181, 182, 183, 300, 362, 363):
        edge = half - k * res  # x of the boundary between rows k-1 and k (exact in double)
        f = np.float32(edge)
        xs += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    xs = np.array(xs, dtype=np.float32)
    X, Y = np.meshgrid(xs, xs)
    pts = np.column_stack([X.ravel(), Y.ravel(), np.full(X.size, -1.7, dtype=np.float32)])
    return Scene("index_fast_path_boundaries", synth.make_cloud(pts), "k_classify index_of: the exactness check at cell boundaries",
                 frames=1)


def index_exact_division() -> Scene:
    """a == 0 exactly: map position chosen so that (x - L/2) - pos == 0 for x = 5 -> the exact-division path"""
    half = 0.5 * oracle.OracleMap(120.0, 0.33).length[0]
    pos = (float(np.float64(np.float32(5.0)) - half), float(np.float64(np.float32(-7.25)) - half))
    pts = np.array([[5.0, -7.25, -1.0], [5.0, -7.0, -1.0], [4.9, -7.25, -1.2], [3.0, -9.0, -1.1]], dtype=np.float32)
    return Scene("index_exact_division", synth.make_cloud(pts), "k_classify index_of: the exact division", pos=pos,
                 origin=(pos[0], pos[1], 0.0), frames=1)


MAP_BORDER_POSITIONS = [(0.0, 0.0), (500000.3, 5800000.7), (-1.0e7, 3.3e6), (9.0e8, -9.9e8), (3.0e9, -2.0e10), (1.0e15, 1.0e15)]


def map_border(pos) -> Scene:
    """isInside and getIndex at the map's four borders: points on, next to and beyond them, at UTM-sized map positions and at
    positions so far out that an ulp of the coordinates is larger than a cell"""
    m = oracle.OracleMap(120.0, 0.33, pos=pos)
    half, res = 0.5 * m.length[0], m.resolution
    offs = []
    for k in (-2, -1, 0, 1, 2, 3, 180, 361, 362, 363, 364, 365):
        for d in (0.0, 1e-7, -1e-7, 0.5 * res):
            offs.append(half - k * res + d)
    offs = np.array(offs + [1e30, -1e30, np.inf, np.nan])
    xs = (np.float64(pos[0]) + offs).astype(np.float32)
    ys = (np.float64(pos[1]) + offs).astype(np.float32)
    X, Y = np.meshgrid(xs, ys)
    pts = np.column_stack([X.ravel(), Y.ravel(), np.full(X.size, -1.7, dtype=np.float32)])
    return Scene(f"map_border_{pos[0]:g}_{pos[1]:g}", synth.make_cloud(pts), "k_classify isInside / index_of at the map border",
                 pos=tuple(pos), origin=(np.float32(pos[0]), np.float32(pos[1]), 0.0), frames=2)


LABEL_TOLERANCE_CONFIGS = [(0.0005, 0.3, 0.1), (2e-5, 0.3, 0.1), (2e-6, 0.3, 0.1), (1e-7, 0.3, 0.1), (0.0005, 0.1, 0.3),
                           (0.0005, 0.0, 0.1), (-0.0005, 0.3, 0.1), (0.02, 0.3, 0.299)]


def label_tolerance_edit(mdf, thres, obs):
    def edit(c):
        c.minimum_distance_factor = mdf
        c.miminum_point_height_threshold = thres
        c.minimum_point_height_obstacle_threshold = obs
    return edit


def label_tolerance(mdf, thres, obs) -> Scene:
    """k_label's clamp of the tolerance (:170-171) from the point's CELL; factors that put most points above the clamp, inside
    the band, below it; thresholds in the unusual order, zero, a negative factor; origin off the map centre"""
    return Scene(f"label_tolerance_{mdf:g}_{thres:g}_{obs:g}", synth.hdl64_cloud(seed=33, n_az=500), "k_label: the tolerance clamp branches",
                 origin=(3.7, -2.2, 0.1), cfg_edit=label_tolerance_edit(mdf, thres, obs))


def random_scene(seed) -> Scene:
    """Random geometry, random clusters (one of them packing tens of thousands of points into a single 16x16 tile), random map
    position / origin / base height, three frames."""
    rng = np.random.default_rng(1000 + seed)
    # (GroundSegmentation::init takes the dimension as size_t: whole metres)
    length, resolution = [(20.0, 0.2), (30.0, 0.25), (40.0, 0.33), (50.0, 0.5), (64.0, 0.33), (80.0, 0.33), (45.0, 0.2), (33.0, 0.25)][
        int(rng.integers(0, 8))]
    n_clusters = int(rng.integers(3, 9))
    parts = []
    for k in range(n_clusters):
        centre = rng.uniform(-0.55 * length, 0.55 * length, size=2)  # some clusters straddle or miss the map
        spread = float(rng.choice([0.05, 0.3, 1.5, 6.0, 20.0]))
        m = int(rng.integers(50, 40000 if k == 0 else 6000))
        xy = centre + rng.normal(0, spread, size=(m, 2))
        z = rng.normal(rng.uniform(-2.5, 0.5), rng.choice([0.0, 0.02, 0.4]), size=m)
        parts.append(np.column_stack([xy, z]))
    pts = np.concatenate(parts).astype(np.float32)
    rng.shuffle(pts)
    pos = tuple(np.round(rng.uniform(-3, 3, size=2), 2))
    origin = (float(pos[0]) + float(rng.uniform(-1, 1)), float(pos[1]) + float(rng.uniform(-1, 1)), float(rng.uniform(-0.2, 0.2)))
    cloud = synth.make_cloud(pts + np.array([pos[0], pos[1], 0.0], np.float32), ring=rng.integers(0, 64, len(pts)))
    return Scene(f"random_{seed}", cloud, "everything, on random geometry", length=length, resolution=resolution, pos=pos, origin=origin,
                 base_z=float(rng.uniform(-2.0, -1.4)), frames=3, odom_z=float(rng.uniform(-0.5, 0.5)))


# ---------------------------------------------------------------- batch-only scenes

BATCH_SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049]


def sized(n, seed=0) -> Scene:
    """exactly n points (around the 64-point chunks of small contexts and the 2048-point chunks of large ones), half of them
    near the sensor so that small clouds still reach dense cells"""
    c = synth.random_cloud(n, seed=7000 + seed + n, extent=30.0)
    return Scene(f"sized_{n}", c, "front end chunking: the cloud ends on / next to a chunk border")


def special_bits() -> Scene:
    """-0.0, subnormal and signalling-NaN coordinates in x, y and z (bit patterns the 16-byte packing and the 32-byte loads must
    carry unchanged), among ordinary returns of the same cells"""
    rng = np.random.default_rng(31)
    n = 96
    xy = rng.uniform(-3.0, 3.0, size=(n, 2))
    z = rng.normal(-1.7, 0.05, n)
    c = synth.make_cloud(np.column_stack([xy, z]).astype(np.float32), ring=rng.integers(0, 64, n))
    bits = {"x": c["x"].view(np.uint32), "y": c["y"].view(np.uint32), "z": c["z"].view(np.uint32)}
    specials = [0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800001, 0xFFA00001, 0x7FBFFFFF]
    k = 0
    for name in ("x", "y", "z"):
        for v in specials:
            bits[name][k] = v
            k += 1
    # -0.0 everywhere in one point and the exact origin in another
    for name in ("x", "y", "z"):
        bits[name][k] = 0x80000000
    c["intensity"] = np.arange(n, dtype=np.float32)
    return Scene("special_bits", c, "pack16 / PointXYZIR loads: -0.0, subnormal and signalling-NaN coordinates", extra={"n_specials": k + 1})


UTM_POSITIONS = [(500000.3, 5800000.7), (683211.5, 5712033.25), (-1.0e7, 3.3e6), (312000.125, 4100000.5)]


def utm_drive(pos, seed) -> Scene:
    """a sensor cloud on a map at a UTM-sized position (the cloud shifted there in float, as a map-frame cloud would be)"""
    base = synth.hdl64_cloud(seed=seed, n_az=120)
    c = synth.clone_cloud(base)
    c["x"] = (base["x"].astype(np.float64) + pos[0]).astype(np.float32)
    c["y"] = (base["y"].astype(np.float64) + pos[1]).astype(np.float32)
    return Scene(f"utm_{pos[0]:g}_{pos[1]:g}", c, "k_classify index_of far from the frame origin", pos=tuple(pos),
                 origin=(np.float32(pos[0]), np.float32(pos[1]), np.float32(0.0)))


def adversarial_scenes():
    """The hostile single-map scenes on the 120 m / 0.33 m grid with the default configuration, in a fixed order."""
    s = [edge_cases(), reduce_recurrence_rare_cases(), exact_tile_records(), line_of_sight_walk(), signalling_nan_heights(), empty(),
         all_outside(), dense_single_cells_and_ties(), reduce_tile_classes_long_cells_and_quotient_fallbacks(), corrupt_z(),
         index_fast_path_boundaries(), index_exact_division(), special_bits()]
    s += [map_border(p) for p in MAP_BORDER_POSITIONS[1:3]]
    s += [utm_drive(p, 40 + k) for k, p in enumerate(UTM_POSITIONS)]
    return s
