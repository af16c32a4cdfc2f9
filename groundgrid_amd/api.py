"""Host-side mirror of the reference's operator interface for the hot path, on top of the C ABI.

``GroundSegmentation`` keeps the names and argument meaning of ``groundgrid::GroundSegmentation``
(/root/reference/include/groundgrid/GroundSegmentation.h:48-71): ``init``, ``setConfig``,
``filter_cloud``.  The grid map the reference borrows by reference (``grid_map::GridMap&``, owned by
``GroundGrid``) lives in HBM inside the context; ``GridMap`` is a handle to one such map ("slot") with
grid_map-like accessors.  ``filter_batch`` is the device-resident batched form (independent
(cloud, map) pairs in one set of launches) used for throughput runs and multi-GPU sharding.

PyTorch is used only for device buffers / streams in the batched path.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import GGBatch, GGConfig, GGGeometry, GroundGridError, LAYERS
from .synth import POINT_DTYPE

# label / class codes (include/groundgrid_hip.h)
DROPPED, GROUND, NONGROUND = 0, 49, 99
OUTSIDE, IGNORED, OUTLIER, KEPT = 0, 1, 2, 3

POINT16_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ring", "<u2"), ("pad", "<u2")])
# the 18-byte sensor_msgs/PointCloud2 record of scripts/kitti_data_publisher.py:139-150
PC2_DTYPE = np.dtype({"names": ["x", "y", "z", "intensity", "ring"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 4, 8, 12, 16], "itemsize": 18})


def to_pc2(cloud: np.ndarray) -> np.ndarray:
    """PointXYZIR (32 B) -> the 18-byte PointCloud2 records a publisher would send."""
    out = np.zeros(cloud.shape[0], dtype=PC2_DTYPE)
    for k in ("x", "y", "z", "intensity", "ring"):
        out[k] = cloud[k]
    return out


def default_config() -> GGConfig:
    c = GGConfig()
    _lib.load().gg_default_config(C.byref(c))
    return c


def transform_from_pose(pose7, rotation: str = "kdl") -> np.ndarray:
    """(tx, ty, tz, qx, qy, qz, qw) -> 3x4 (R | t) with the rotation built the way tf2::Matrix3x3::setRotation ("tf2") or
    KDL::Rotation::Quaternion ("kdl": what doTransform(PointStamped) goes through in ROS Noetic) builds it."""
    p = (C.c_double * 7)(*[float(v) for v in pose7])
    out = (C.c_double * 12)()
    rc = _lib.load().gg_transform_from_pose(_lib.ROTATION[rotation], p, out)
    if rc != _lib.GG_OK:
        raise GroundGridError(f"gg_transform_from_pose: {_lib.STATUS.get(rc, rc)}")
    return np.array(list(out), dtype=np.float64).reshape(3, 4)


def pack16(cloud: np.ndarray) -> np.ndarray:
    """PointXYZIR (32 B) -> packed 16-B device records (x, y, z, ring)."""
    out = np.zeros(cloud.shape[0], dtype=POINT16_DTYPE)
    out["x"], out["y"], out["z"], out["ring"] = cloud["x"], cloud["y"], cloud["z"], cloud["ring"]
    return out


def _check(L, ctx, rc, what):
    if rc != _lib.GG_OK:
        msg = L.gg_last_error(ctx).decode() if ctx else ""
        raise GroundGridError(f"{what}: {_lib.STATUS.get(rc, rc)} {msg}")


# -- the argument frame of the methods over the device calls: the plane methods (fuse_states, route_planes, match_planes, footprint_planes,
# route_headings, score_rollouts, track_clusters), the transfers (export_layers, export_slopes, import_layers), export_images and the cloud methods

def _name_mask(who, names, known, ordered, unknown=None, empty_ok=False):
    """(names as a list, their bit mask): distinct names of `known`, in its order.  ordered: the text when they are not -- or, unless
    empty_ok, when none is named.  unknown: what the text calls a name that is not known; None leaves it to list.index's ValueError."""
    names = list(names)
    strangers = [k for k in names if k not in known]
    if strangers and unknown:
        raise ValueError(f"{who}: unknown {unknown} {strangers}; known: {list(known)}")
    mask = sum(1 << known.index(k) for k in names)
    if [k for k in known if k in names] != names or not (names or empty_ok):
        raise ValueError(f"{who}: {ordered}")
    return names, mask


_LAYER_NAMES = (LAYERS, "names must be distinct and in gg_layer order", None, True)
_SLOPE_NAMES = (_lib.SLOPE_CHANNELS, "names must be distinct and in GG_SLOPE_* order", "channels")


def _occupancy(who, min_points, min_height, max_height):
    """the thresholds of an occupied cell, checked: (min_points, min_height, max_height)"""
    if int(min_points) < 1:
        raise ValueError(f"{who}: min_points < 1")
    if math.isnan(float(min_height)) or math.isnan(float(max_height)):
        raise ValueError(f"{who}: min_height or max_height is NaN")
    return int(min_points), float(min_height), float(max_height)


def _max_cells(who, max_cells):
    if int(max_cells) != max_cells or int(max_cells) < 0 or int(max_cells) > 0x7FFFFFFF:
        raise ValueError(f"{who}: max_cells is an integer >= 0")
    return int(max_cells)


def _plane_order(who, order, rows, cols):
    """`order` checked: (the shape of one plane, GG_PLANES_*)"""
    if order not in ("row", "col"):
        raise ValueError(f"{who}: order is 'row' or 'col'")
    return ((rows, cols), _lib.GG_PLANES_ROWMAJOR) if order == "row" else ((cols, rows), _lib.GG_PLANES_COLMAJOR)


def _check_integers(who, **named):
    for name, v in named.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: {name} is an integer")


def _is_dense(t, shape, dtype=None, device=None):
    """a contiguous CUDA tensor of that shape and dtype (None: torch.int32), on `device` where one is named"""
    import torch

    return (torch.is_tensor(t) and t.is_cuda and t.dtype == (dtype or torch.int32) and tuple(t.shape) == shape and t.is_contiguous()
            and (device is None or t.device == device))


def _is_planes(t, plane):
    """a contiguous CUDA torch.int32 tensor [B, *plane]"""
    import torch

    return torch.is_tensor(t) and t.dim() == 3 and _is_dense(t, (int(t.shape[0]),) + plane)


def _int32_array(who, name, given, shape_text, ok, suffix=""):
    """anything np.asarray turns into exact int32 of a shape that `ok` accepts, as a contiguous host array"""
    try:
        given = np.asarray(given)
        host = np.ascontiguousarray(given.astype(np.int32))
        exact = given.shape == host.shape and np.array_equal(given, host)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"{who}: {name} must be {shape_text} int32: {e}") from None
    if not ok(host.shape) or not exact:
        raise ValueError(f"{who}: {name} of shape {host.shape} are not {shape_text} int32{suffix}")
    return host


def _int32_ptr(host):
    return host.ctypes.data_as(C.POINTER(C.c_int32))


def _reuse_outputs(who, res, want, device, inputs=(), fill=None, in_place="is an input of the call: no update in place is defined"):
    """The structured `out` of a method.  want: {field of res: shape (of an int32 tensor), (shape, dtype), or None for a field not asked
    for}.  A tensor that res holds must be asked for, be of that dtype and shape on `device`, and start at none of the `inputs`
    (data_ptr()s); nothing is allocated before every field has passed, then the missing ones are (fill: {field: the word a fresh
    tensor is filled with})."""
    import torch

    want = {field: spec if spec is None or isinstance(spec[-1], torch.dtype) else (spec, torch.int32) for field, spec in want.items()}
    for field, spec in want.items():
        t = getattr(res, field)
        if spec is None:
            if t is not None:
                raise ValueError(f"{who}: out.{field} is given but not asked for")
        elif t is not None:
            if not _is_dense(t, *spec, device):
                raise ValueError(f"{who}: out.{field} must be a contiguous CUDA {spec[1]} tensor of shape {spec[0]}")
            if t.data_ptr() in inputs:
                raise ValueError(f"{who}: out.{field} {in_place}")
    for field, spec in want.items():
        if spec is not None and getattr(res, field) is None:
            if fill and field in fill:
                setattr(res, field, torch.full(spec[0], fill[field], dtype=spec[1], device=device))
            else:
                setattr(res, field, torch.empty(spec[0], dtype=spec[1], device=device))
    return res


class GridMap:
    """Handle to one device-resident map state (the reference's grid_map::GridMap with its 11 layers)."""

    def __init__(self, seg: "GroundSegmentation", slot: int):
        self._seg = seg
        self.slot = slot
        self._pos = (0.0, 0.0)

    # grid_map-like accessors
    def getSize(self):
        return self._seg.rows, self._seg.cols

    def getResolution(self) -> float:
        return self._seg.resolution

    def getLength(self):
        return self._seg.length

    def getPosition(self):
        return self._pos

    def setConfig(self, config: Optional[GGConfig]):
        """This map's own configuration (GroundSegmentation::setConfig of the reference's object for this map); None: follow the
        context's configuration again."""
        self._seg.set_slot_configs(None if config is None else [config], slots=[self.slot])

    def getConfig(self) -> GGConfig:
        return self._seg.slot_config(self.slot)[0]

    def setPosition(self, x: float, y: float):
        """Map position after grid_map::move (src/GroundGrid.cpp:97)."""
        L, ctx = self._seg._L, self._seg._ctx
        _check(L, ctx, L.gg_set_map_position(ctx, self.slot, float(x), float(y)), "gg_set_map_position")
        self._pos = (float(x), float(y))

    def move(self, odom_x: float, odom_y: float, base_to_map=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), rotation: str = "kdl"):
        """GroundGrid::update (src/GroundGrid.cpp:83-147) on the device.  base_to_map = (tx, ty, tz, qx, qy, qz, qw) of
        lookupTransform("base_link", "map"); `rotation` picks the quaternion -> matrix convention of doTransform (the ABI
        itself takes the matrix entries).  Returns the index shift (rows, cols)."""
        L, ctx = self._seg._L, self._seg._ctx
        M = transform_from_pose(base_to_map, rotation)
        plane = (C.c_double * 4)(M[2, 0], M[2, 1], M[2, 2], M[2, 3])
        sh = (C.c_int * 2)()
        _check(L, ctx, L.gg_move_map(ctx, self.slot, float(odom_x), float(odom_y), plane, sh), "gg_move_map")
        x, y = C.c_double(), C.c_double()
        L.gg_get_map_position(ctx, self.slot, C.byref(x), C.byref(y))
        self._pos = (x.value, y.value)
        return sh[0], sh[1]

    def reset(self, odom_z: float = 0.0, pos=(0.0, 0.0)):
        """GroundGrid::initGroundGrid layer values (src/GroundGrid.cpp:71-75)."""
        L, ctx = self._seg._L, self._seg._ctx
        _check(L, ctx, L.gg_reset_map(ctx, self.slot, float(pos[0]), float(pos[1]), C.c_float(odom_z)), "gg_reset_map")
        self._pos = (float(pos[0]), float(pos[1]))

    def get(self, layer: str) -> np.ndarray:
        """Layer as a (rows, cols) float32 array (element (i, j) == Eigen's matrix(i, j))."""
        L, ctx = self._seg._L, self._seg._ctx
        buf = np.empty(self._seg.rows * self._seg.cols, dtype=np.float32)
        _check(L, ctx, L.gg_get_layer(ctx, self.slot, LAYERS.index(layer), buf.ctypes.data), "gg_get_layer")
        return buf.reshape((self._seg.rows, self._seg.cols), order="F")

    __getitem__ = get

    def set(self, layer: str, arr: np.ndarray):
        L, ctx = self._seg._L, self._seg._ctx
        a = np.asfortranarray(np.asarray(arr, dtype=np.float32))
        assert a.shape == (self._seg.rows, self._seg.cols)
        flat = np.ascontiguousarray(a.reshape(-1, order="F"))
        _check(L, ctx, L.gg_set_layer(ctx, self.slot, LAYERS.index(layer), flat.ctypes.data), "gg_set_layer")

    def layers(self, names=None) -> dict:
        """All (or the named) layers with one synchronisation (gg_get_layers): what a publisher loop reads after a cloud."""
        L, ctx = self._seg._L, self._seg._ctx
        names = list(LAYERS) if names is None else list(names)
        n = self._seg.rows * self._seg.cols
        bufs = {k: np.empty(n, dtype=np.float32) for k in names}
        ptrs = (C.c_void_p * len(LAYERS))(*[bufs[k].ctypes.data if k in bufs else None for k in LAYERS])
        _check(L, ctx, L.gg_get_layers(ctx, self.slot, ptrs), "gg_get_layers")
        return {k: v.reshape((self._seg.rows, self._seg.cols), order="F") for k, v in bufs.items()}

    def image_u8(self, layer: str):
        """GridMapCvConverter::toImage<unsigned char,1> (Nodelet.cpp:239): (rows x cols uint8 image, lower, upper)."""
        L, ctx = self._seg._L, self._seg._ctx
        img = np.empty((self._seg.rows, self._seg.cols), dtype=np.uint8)
        lo, hi = C.c_float(), C.c_float()
        _check(L, ctx, L.gg_get_layer_image_u8(ctx, self.slot, LAYERS.index(layer), img.ctypes.data, C.byref(lo), C.byref(hi)), "gg_get_layer_image_u8")
        return img, lo.value, hi.value

    def gridmap_message(self, layers=None, seq: int = 0, stamp=(0, 0), frame_id: str = "map", basic_layers=()) -> bytes:
        """The serialised grid_map_msgs/GridMap the nodelet publishes per cloud (Nodelet.cpp:211-214), ROS 1 wire format."""
        L, ctx = self._seg._L, self._seg._ctx
        mask = 0 if layers is None else sum(1 << LAYERS.index(k) for k in layers)
        hdr = _lib.GGGridMapHeader(int(seq), int(stamp[0]), int(stamp[1]), frame_id.encode(), sum(1 << LAYERS.index(k) for k in basic_layers))
        size = C.c_size_t(0)
        _check(L, ctx, L.gg_get_gridmap_message(ctx, self.slot, mask, C.byref(hdr), None, 0, C.byref(size)), "gg_get_gridmap_message")
        buf = np.empty(size.value, dtype=np.uint8)
        _check(L, ctx, L.gg_get_gridmap_message(ctx, self.slot, mask, C.byref(hdr), buf.ctypes.data, buf.size, C.byref(size)), "gg_get_gridmap_message")
        return buf.tobytes()

    # -- the stage members of the reference's class on this map as it stands (include/groundgrid/GroundSegmentation.h:59-62)
    def _stage(self, stage, section=0, i=0, j=0, base_z=0.0):
        L, ctx = self._seg._L, self._seg._ctx
        args = _lib.GGStageArgs(int(section), int(i), int(j), float(base_z))
        _check(L, ctx, L.gg_run_stage(ctx, self.slot, stage, C.byref(args)), "gg_run_stage")

    def detect_ground_patches(self, section: int = -1):
        """detect_ground_patches(map, section) (:314-340): section 0..3, or -1 for all four quadrants."""
        self._stage(_lib.GG_STAGE_DETECT_GROUND_PATCHES, section=section)

    def detect_ground_patch(self, S: int, i: int, j: int):
        assert S in (3, 5)
        self._stage(_lib.GG_STAGE_DETECT_GROUND_PATCH_3 if S == 3 else _lib.GG_STAGE_DETECT_GROUND_PATCH_5, i=i, j=j)

    def spiral_ground_interpolation(self, toBase_z: float):
        self._stage(_lib.GG_STAGE_SPIRAL_GROUND_INTERPOLATION, base_z=toBase_z)

    def interpolate_cell(self, x: int, y: int):
        self._stage(_lib.GG_STAGE_INTERPOLATE_CELL, i=x, j=y)

    def insert_cloud(self, cloud: np.ndarray, start: int, end: int, cloudOrigin: Sequence[float]):
        """GroundSegmentation::insert_cloud(cloud, start, end, cloudOrigin, point_index, ignored, outliers, map)
        (include/groundgrid/GroundSegmentation.h:55, src/GroundSegmentation.cpp:200-311) on this map as it stands (no per-call reset).
        Returns (class, cell) per point of [start, end) in cloud order; the three lists the reference appends to are the points of class
        KEPT / IGNORED (with their cells) / OUTLIER in that order."""
        L, ctx = self._seg._L, self._seg._ctx
        cloud = np.ascontiguousarray(cloud)
        assert cloud.dtype.itemsize == 32 and 0 <= start <= end <= len(cloud)
        n = end - start
        cls, cell = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int32)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        _check(L, ctx, L.gg_insert_cloud(ctx, self.slot, cloud.ctypes.data, start, end, org, cls.ctypes.data, cell.ctypes.data), "gg_insert_cloud")
        return cls, cell

    def scores(self, allow_unknown: bool = False):
        """This map's evaluator (GroundSegmentation.scores for one slot)."""
        return self._seg.scores(slots=[self.slot], allow_unknown=allow_unknown)[0]

    def terrain_image(self) -> np.ndarray:
        """The 32FC3 terrain image of Nodelet.cpp:247-268: rows x cols x (ground, visited flag, pointsRaw)."""
        L, ctx = self._seg._L, self._seg._ctx
        img = np.empty((self._seg.rows, self._seg.cols, 3), dtype=np.float32)
        _check(L, ctx, L.gg_get_terrain_image(ctx, self.slot, img.ctypes.data), "gg_get_terrain_image")
        return img


@dataclass
class BatchOutputs:
    labels: "object"      # torch.uint8 [B, stride]
    out_index: "object"   # torch.int32 [B, stride]
    counts: "object"      # torch.int32 [B, 4]: returned size, kept, ignored, outliers
    out_clouds: "object" = None
    label_masks: "object" = None  # torch.uint8 [B, stride // 4]: 2 bits per point (0 dropped, 1 ground, 2 non-ground)
    out_pc2: "object" = None      # torch.uint8 [B, stride * 18]: the returned clouds as 18-byte PointCloud2 records


@dataclass
class ImageExport:
    """what GroundSegmentation.export_images returns (CUDA torch tensors; None where nothing was asked for)"""

    images: "object" = None   # torch.uint8 [n, K, rows, cols]
    bounds: "object" = None   # torch.float32 [n, K, 2]: lower, upper
    terrain: "object" = None  # torch.float32 [n, rows, cols, 3], or [n, 3, rows, cols] with chw


@dataclass
class SplitOutputs:
    """what GroundSegmentation.split_clouds returns (CUDA torch tensors; None where nothing was asked for).  Row i of every tensor belongs to
    cloud i; only its first counts[i, 0] (ground) / counts[i, 1] (nonground) elements are written."""

    counts: "object" = None            # torch.int32 [n, 2]: points in ground, in nonground
    ground_points: "object" = None     # torch.uint8 [n, stride, 16]: packed gg_point16 (x, y, z in the map frame, ring, pad = 0)
    ground_height: "object" = None     # torch.float32 [n, stride]: z - ground(cell of the point)
    ground_source: "object" = None     # torch.int32 [n, stride]: index of the point in its input cloud
    nonground_points: "object" = None
    nonground_height: "object" = None
    nonground_source: "object" = None

    def clouds(self, which: str = "nonground"):
        """The rows of set `which` ("ground" / "nonground") trimmed to their counts: a list of (points, height, source) views, one per
        cloud (None for a tensor that was not asked for).  The ONE place that synchronises: it reads `counts` on the host."""
        col = {"ground": 0, "nonground": 1}[which]
        sizes = self.counts[:, col].cpu().tolist()
        fields = [getattr(self, f"{which}_{k}") for k in ("points", "height", "source")]
        return [tuple(None if t is None else t[i, :m] for t in fields) for i, m in enumerate(sizes)]


# gg_cluster as a numpy record (ClusterOutputs.table)
CLUSTER_DTYPE = np.dtype([("cells", "<i4"), ("points", "<i4"), ("row_min", "<i4"), ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4"),
                          ("height_max", "<f4"), ("first_cell", "<i4")])


@dataclass
class ClusterOutputs:
    """what GroundSegmentation.cluster_clouds returns (CUDA torch tensors; None where nothing was asked for)"""

    cell_cluster: "object" = None   # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): -1 or the cell's cluster id
    n_clusters: "object" = None     # torch.int32 [B]: the true number of clusters of every cloud
    clusters: "object" = None       # torch.int32 [B, max_clusters, 8]: gg_cluster records (word 6 holds the bits of the float height_max)
    point_cluster: "object" = None  # torch.int32 [B, stride]: -1 or the id of the point's cell, for p < n_points[b]

    def table(self, b: int):
        """The first min(K, max_clusters) records of cloud b as a numpy structured array (CLUSTER_DTYPE, height_max as float32).  The ONE
        place that synchronises: it reads the count on the host."""
        k = min(int(self.n_clusters[b].item()), int(self.clusters.shape[1]))
        return self.clusters[b, :k].cpu().numpy().copy().view(CLUSTER_DTYPE).reshape(k)


@dataclass
class ClearanceOutputs:
    """what GroundSegmentation.clearance_clouds and clearance_planes return (CUDA torch tensors [B, rows, cols], [B, cols, rows] with
    order="col"; None where nothing was asked for)"""

    dist2: "object" = None       # torch.int32: the squared distance, in cells, to the nearest occupied cell; _lib.GG_CLEARANCE_NONE: none
    nearest: "object" = None     # torch.int32: the linear index, in `order`, of that cell; -1: none
    distance: "object" = None    # torch.float32: sqrt(dist2) * resolution, in metres; +inf: none
    n_occupied: "object" = None  # torch.int32 [B]: the occupied cells of every map


@dataclass
class VisibilityOutputs:
    """what GroundSegmentation.visibility_clouds returns (CUDA torch tensors; None where nothing was asked for)"""

    state: "object" = None   # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): _lib.GG_CELL_FREE / _UNKNOWN / _OCCUPIED = -1 / 0 / 1
    counts: "object" = None  # torch.int32 [B, 3]: the free, unknown and occupied cells of every map


@dataclass
class FusionOutputs:
    """what GroundSegmentation.fuse_states returns (CUDA torch tensors; None where nothing was asked for)"""

    evidence: "object" = None  # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): the evidence to hand to the next call
    state: "object" = None     # torch.int32, same shape: _lib.GG_CELL_FREE / _UNKNOWN / _OCCUPIED = -1 / 0 / 1 by the two thresholds
    frontier: "object" = None  # torch.int32, same shape: 0 on a free cell with an unknown neighbour, -1 elsewhere
    counts: "object" = None    # torch.int32 [B, 4]: the free, unknown, occupied and frontier cells of every map


@dataclass
class RouteOutputs:
    """what GroundSegmentation.route_planes returns (CUDA torch tensors; None where nothing was asked for)"""

    dist: "object" = None      # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): the cost to the nearest goal, _lib.GG_ROUTE_NONE where none is reached
    next: "object" = None      # torch.int32, same shape: the linear index (in `order`) of the next cell of the cheapest path; own index on a goal, -1 unreached
    counts: "object" = None    # torch.int32 [B, 3]: the goals, the reached cells (goals included) and the unblocked cells of every map
    paths: "object" = None     # torch.int32 [B, max_path]: the cells of the path from starts[i]; the words from path_len[i] on are never written
    path_len: "object" = None  # torch.int32 [B]: the cells of the whole path, also beyond max_path; 0: no start, or an unreached one


@dataclass
class MatchOutputs:
    """what GroundSegmentation.match_planes returns (CUDA torch tensors; None where nothing was asked for)"""

    best: "object" = None    # torch.int32 [B, 6]: k*, dy*, dx*, S*, the scan cells of the map, the candidates whose score equals S*
    scores: "object" = None  # torch.int32 [B, K, 2 W + 1, 2 W + 1]: S(k, dy, dx) at [k, dy + W, dx + W]


def rotation_table(angles_rad):
    """The yaw candidates of GroundSegmentation.match_planes from angles in radians: int32 [K, 2], row k = (cq, sq) = (16384 cos, 16384 sin)
    of angles_rad[k], each rounded half away from zero, computed in float64.  A positive angle turns the row axis towards the column axis:
    (dr, dc) = (1, 0) goes to (cos, sin).  List the prior yaw (0.0) first: among equal scores the earlier candidate wins."""
    a = np.atleast_1d(np.asarray(angles_rad, dtype=np.float64))
    if a.ndim != 1 or not np.isfinite(a).all():
        raise ValueError("rotation_table: angles_rad is a list of finite angles")
    v = np.stack([np.cos(a), np.sin(a)], axis=1) * float(_lib.GG_MATCH_UNIT)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


@dataclass
class FootprintOutputs:
    """what GroundSegmentation.footprint_planes returns (CUDA torch tensors; None where nothing was asked for)"""

    mask: "object" = None    # torch.int32 [B, rows, cols]: bit k set iff heading k fits at the cell (the uint32 word of gg_footprint_planes, same bits)
    fit: "object" = None     # torch.int32 [B, rows, cols]: -1 where at least min_fit headings fit, else the number that fit
    counts: "object" = None  # torch.int32 [B, 3]: cells where all K headings fit, where at least min_fit fit, where none fits


def footprint_spans(rotations, ahead, behind, left, right, *, pad=0.7072, radius=None):
    """The span table of a rectangular vehicle for GroundSegmentation.footprint_planes (gg_footprint_spans): int32 [K, 2 R + 1, 2], row
    a + R of heading k = (lo, hi), the cells (a, lo .. hi) of the footprint, (1, 0) for an empty row.  rotations: rotation_table(angles),
    int32 [K, 2] with 1 <= K <= 32: the forward axis of heading k is (cq, sq) in (row, col).  The rectangle reaches `ahead` cells along the
    forward axis from the reference cell and `behind` cells against it, `left` cells along the axis a quarter turn from forward (the turn
    that takes the row axis to the column axis) and `right` cells against that; all four >= 0 give a rectangle that holds the reference
    cell, negative values move it off.  A cell belongs to the footprint when its centre lies in the rectangle grown by `pad` cells on
    every side; the default, just over half a cell diagonal, catches every cell the rectangle touches (a choice of this layer alone:
    the C call takes the padded rectangle).  Lengths become units of 1/16384 cell, rounded half away from zero as rotation_table
    rounds.  radius=None takes the smallest radius that holds every heading; ValueError when that exceeds 32 or the radius given."""
    who = "footprint_spans"
    try:
        given = np.asarray(rotations)
        rot = np.ascontiguousarray(given.astype(np.int32))
        exact = given.shape == rot.shape and np.array_equal(given, rot)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"{who}: rotations must be [K, 2] int32: {e}") from None
    if rot.ndim != 2 or rot.shape[1] != 2 or not exact or not 1 <= rot.shape[0] <= _lib.GG_FOOTPRINT_MAX_HEADINGS:
        raise ValueError(f"{who}: rotations are [K, 2] int32 with 1 <= K <= {_lib.GG_FOOTPRINT_MAX_HEADINGS}")
    lengths = [float(v) for v in (ahead, behind, left, right, pad)]
    if not all(math.isfinite(v) for v in lengths):
        raise ValueError(f"{who}: ahead, behind, left, right and pad are finite lengths in cells")
    ahead, behind, left, right, pad = lengths

    def q14(v):
        m = math.floor(abs(v) * float(_lib.GG_MATCH_UNIT) + 0.5)
        return -m if v < 0 else m

    rect = [q14(-(behind + pad)), q14(ahead + pad), q14(-(right + pad)), q14(left + pad)]
    if any(abs(v) > _lib.GG_FOOTPRINT_RECT_LIMIT for v in rect) or rect[0] > rect[1] or rect[2] > rect[3]:
        raise ValueError(f"{who}: the padded rectangle {rect} (1/16384 cell) is empty or reaches beyond 2^30")
    if radius is not None and (isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= _lib.GG_FOOTPRINT_MAX_RADIUS):
        raise ValueError(f"{who}: radius is an integer in [0, {_lib.GG_FOOTPRINT_MAX_RADIUS}] or None")
    L = _lib.load()
    K = rot.shape[0]
    c_rot, c_rect, needed = rot.ctypes.data_as(C.POINTER(C.c_int32)), (C.c_int32 * 4)(*rect), C.c_int(0)
    rc = L.gg_footprint_spans(c_rot, K, c_rect, 0, None, C.byref(needed))
    if rc != _lib.GG_OK:
        raise GroundGridError(f"gg_footprint_spans: {_lib.STATUS.get(rc, rc)}")
    R = max(needed.value, 0) if radius is None else int(radius)
    if needed.value > R or R > _lib.GG_FOOTPRINT_MAX_RADIUS:
        raise ValueError(f"{who}: the footprint needs radius {needed.value}{' or more' if needed.value > _lib.GG_FOOTPRINT_MAX_RADIUS else ''}, "
                         f"beyond {'the largest radius' if radius is None else 'the radius given,'} {min(R, _lib.GG_FOOTPRINT_MAX_RADIUS) if radius is None else R}")
    spans = np.zeros((K, 2 * R + 1, 2), dtype=np.int32)
    rc = L.gg_footprint_spans(c_rot, K, c_rect, R, spans.ctypes.data_as(C.POINTER(C.c_int32)), None)
    if rc != _lib.GG_OK:
        raise GroundGridError(f"gg_footprint_spans: {_lib.STATUS.get(rc, rc)}")
    return spans


@dataclass
class HeadingOutputs:
    """what GroundSegmentation.route_headings returns (CUDA torch tensors; None where nothing was asked for)"""

    dist: "object" = None          # torch.int32 [B, K, rows, cols] ([B, K, cols, rows] with order="col"): the cost to a goal state, _lib.GG_ROUTE_NONE where none is reached
    next: "object" = None          # torch.int32, same shape: the slot of the move to take; _lib.GG_HEADINGS_AT_GOAL on a goal state, -1 unreached
    best: "object" = None          # torch.int32 [B, rows, cols]: the least dist over the headings of a cell
    best_heading: "object" = None  # torch.int32 [B, rows, cols]: the smallest heading that attains it, -1 where none is reached
    counts: "object" = None        # torch.int32 [B, 3]: the goal states, the reached states (goal states included) and the admissible states of every map
    paths: "object" = None         # torch.int32 [B, max_len, 2]: the (cell, heading) pairs of the path from starts[i]; the pairs from path_len[i] on are never written
    path_len: "object" = None      # torch.int32 [B]: the states of the whole path, also beyond max_len; 0: no start, or an unreached one


# gg_track as a numpy record (TrackOutputs.table)
TRACK_DTYPE = np.dtype([("track_id", "<i4"), ("age", "<i4"), ("prev", "<i4"), ("overlap", "<i4"), ("still", "<i4"), ("cells", "<i4"),
                        ("sum_row", "<i4"), ("sum_col", "<i4")])


@dataclass
class TrackOutputs:
    """what GroundSegmentation.track_clusters returns (CUDA torch tensors; None where nothing was asked for) -- and what the next frame's
    call takes as `previous`"""

    tracks: "object" = None        # torch.int32 [B, max_clusters, 8]: gg_track records; only the first heads[b, 1] of map b are written
    heads: "object" = None         # torch.int32 [B, 4]: the next fresh id, the clusters of this scan, the tracks born, the tracks ended
    cell_track: "object" = None    # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): the cell's track id, -1 on a cell of no cluster
    cell_cluster: "object" = None  # the id planes the call was given (kept alive for the next frame, which reads them as its previous scan)
    order: str = "row"

    def table(self, b: int):
        """The heads[b, 1] records of map b as a numpy structured array (TRACK_DTYPE).  It synchronises: it reads the head on the host."""
        k = min(max(int(self.heads[b, 1].item()), 0), int(self.tracks.shape[1]))
        return self.tracks[b, :k].cpu().numpy().copy().view(TRACK_DTYPE).reshape(k)

    def motion(self, previous: "TrackOutputs", shifts=None, resolution: float = 1.0):
        """A host convenience, not part of the bit contract: the displacement of every cluster's centroid since `previous` (the
        TrackOutputs this one was computed from) with the map's own move taken out, float64 [B, max_clusters, 2] in metres, (dx, dy) in
        the map frame (a row index grows towards -x and a column index towards -y, as in grid_map); NaN for a cluster that continues
        nothing and for the records beyond heads[b, 1].  shifts: what the call was given, [B, 2] or None.  It synchronises."""
        cur, old = self.tracks.cpu().numpy(), previous.tracks.cpu().numpy()
        n_cur = self.heads[:, 1].cpu().numpy()
        B, M = cur.shape[:2]
        s = np.zeros((B, 2), dtype=np.float64) if shifts is None else np.asarray(shifts, dtype=np.float64).reshape(B, 2)
        out = np.full((B, M, 2), np.nan, dtype=np.float64)
        for b in range(B):
            rec = cur[b, :min(max(int(n_cur[b]), 0), M)]
            k = np.nonzero(rec[:, 2] >= 0)[0]
            if k.size == 0:
                continue
            pre = old[b, rec[k, 2]]
            here = rec[k, 6:8] / rec[k, 5:6].astype(np.float64) + s[b]   # in the previous scan's index frame
            there = pre[:, 6:8] / pre[:, 5:6].astype(np.float64)
            out[b, k] = -(here - there) * float(resolution)
        return out


BOX_DTYPE = np.dtype([("heading", "<i4"), ("points", "<i4"), ("a_min", "<i4"), ("a_max", "<i4"), ("b_min", "<i4"), ("b_max", "<i4"),
                      ("cost_lo", "<i4"), ("cost_hi", "<i4")])


@dataclass
class BoxOutputs:
    """what GroundSegmentation.box_clusters returns (CUDA torch tensors; None where nothing was asked for)"""

    boxes: "object" = None  # torch.int32 [B, max_clusters, 8]: gg_box records; only the first min(max(n_clusters[b], 0), max_clusters) of cloud b are written
    costs: "object" = None  # torch.int64 [B, max_clusters, K]: the bits of the uint64 cost of every (cluster, heading); -1 (all ones): no point

    def metric(self, b: int, rotations, resolution: float, position=(0.0, 0.0)):
        """A host convenience, not part of the bit contract: the rectangles of cloud b in metres, float64 [max_clusters, 5] = centre x,
        centre y (map frame), length (along the heading), width (across it) and yaw = atan2(sq, cq) of the chosen table entry; NaN for a
        record without a heading (its words may be whatever the tensor held).  rotations: the table the call was given; resolution and
        position: the map's.  The centre of the box in (a, b) is rotated back by the transpose of the heading and moved by half a unit
        for the floor of the quantisation.  It synchronises."""
        rec = self.boxes[b].cpu().numpy().astype(np.int64)
        rot = np.asarray(rotations, dtype=np.int64).reshape(-1, 2)
        out = np.full((rec.shape[0], 5), np.nan, dtype=np.float64)
        ok = (rec[:, 0] >= 0) & (rec[:, 0] < rot.shape[0])
        k = rec[ok, 0]
        unit = float(resolution) / float(_lib.GG_BOX_UNIT)       # metres per unit
        q = float(_lib.GG_MATCH_UNIT)
        cq, sq = rot[k, 0] / q, rot[k, 1] / q
        ca, cb = 0.5 * (rec[ok, 2] + rec[ok, 3]) / q, 0.5 * (rec[ok, 4] + rec[ok, 5]) / q  # the centre, in units, in the heading's frame
        out[ok, 0] = float(position[0]) + (ca * cq - cb * sq + 0.5) * unit
        out[ok, 1] = float(position[1]) + (ca * sq + cb * cq + 0.5) * unit
        out[ok, 2] = (rec[ok, 3] - rec[ok, 2]) / q * unit
        out[ok, 3] = (rec[ok, 5] - rec[ok, 4]) / q * unit
        out[ok, 4] = np.arctan2(sq, cq)
        return out


# gg_region as a numpy record (RegionOutputs.table), 48 bytes
REGION_DTYPE = np.dtype([("cells", "<i4"), ("row_min", "<i4"), ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4"), ("first_cell", "<i4"),
                         ("value_cell", "<i4"), ("value_min", "<i4"), ("sum_row", "<i8"), ("sum_col", "<i8")])


@dataclass
class RegionOutputs:
    """what GroundSegmentation.cluster_planes returns (CUDA torch tensors; None where nothing was asked for)"""

    cell_cluster: "object" = None  # torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): -1 or the id of the cell's kept region
    cell_size: "object" = None     # torch.int32 [B, rows, cols]: 0 on a non-member, else the size of the cell's component, dropped ones too
    heads: "object" = None         # torch.int32 [B, 4]: K, dropped components, member cells, kept cells
    regions: "object" = None       # torch.int32 [B, max_regions, 12]: gg_region records; only the first min(heads[b, 0], max_regions) of map b are written

    def table(self, b: int):
        """The first min(K, max_regions) records of map b as a numpy structured array (REGION_DTYPE).  It synchronises: it reads the
        count on the host."""
        k = min(max(int(self.heads[b, 0].item()), 0), int(self.regions.shape[1]))
        return self.regions[b, :k].cpu().numpy().copy().view(REGION_DTYPE).reshape(k)

    def centroids(self, b: int, resolution: float, length, position=(0.0, 0.0)):
        """A host convenience, not part of the bit contract: the centroids of map b's regions in metres in the map frame, float64 [k, 2]
        = (x, y), by grid_map's rule for the centre of a cell (a row index grows towards -x and a column index towards -y from the
        corner position + length / 2).  resolution, length = (length_x, length_y) and position: the map's.  It synchronises."""
        t = self.table(b)
        n = np.maximum(t["cells"].astype(np.float64), 1.0)
        out = np.empty((t.shape[0], 2), dtype=np.float64)
        out[:, 0] = float(position[0]) + 0.5 * float(length[0]) - (t["sum_row"] / n + 0.5) * float(resolution)
        out[:, 1] = float(position[1]) + 0.5 * float(length[1]) - (t["sum_col"] / n + 0.5) * float(resolution)
        return out


# a record of gg_score_rollouts as a numpy record (RolloutOutputs.table)
ROLLOUT_DTYPE = np.dtype([("steps", "<i4"), ("len", "<i4"), ("cost", "<i4"), ("end_cell", "<i4"), ("end_heading", "<i4"), ("togo", "<i4"),
                          ("clear", "<i4"), ("total", "<i4")])


@dataclass
class RolloutOutputs:
    """what GroundSegmentation.score_rollouts returns (CUDA torch tensors; None where nothing was asked for)"""

    records: "object" = None  # torch.int32 [B, P, 8]: steps, len, cost, end_cell, end_heading, togo, clear, total of every rollout
    best: "object" = None     # torch.int32 [B, 4]: the best rollout (-1: none), its total, the complete rollouts, the scored rollouts
    step_major: "object" = None  # the step-major table the call read (kept alive until the stream has passed the call)

    def table(self, b: int):
        """The P records of map b as a numpy structured array (ROLLOUT_DTYPE).  It synchronises: it reads the records on the host."""
        return self.records[b].cpu().numpy().copy().view(ROLLOUT_DTYPE).reshape(-1)


def rollout_arcs(rotations, speeds, turns, steps: int, unit: int = 10):
    """A library of constant-curvature arcs for GroundSegmentation.score_rollouts in the relative frame: int32 [P, T, 4] with
    P = len(speeds) * len(turns), T = steps, rollout p = i * len(turns) + j pairing speeds[i] with turns[j].  A host convenience, not
    part of the bit contract.  What it computes, in float64:
      speeds[i] = v, cells per step along the heading (negative: backwards); turns[j] = w, radians per step (positive turns the forward
      axis towards the side axis, as rotation_table).  After step t (t = 0 .. T - 1) the heading has turned by phi = (t + 1) * w and the
      pose lies at (a, b) = (v / w) * (sin phi, 1 - cos phi) in (forward, side) cells, (v * (t + 1), 0) when w == 0.
      da, db = 16 * a, 16 * b, each rounded half away from zero (units of 1/16 cell).
      dk = the entry k of `rotations` (int32 [K, 2] as of rotation_table, 1 <= K <= 32) whose angle atan2(sq_k, cq_k) - atan2(sq_0, cq_0)
      lies nearest to phi on the circle; among equally near entries the smallest k.  0 <= dk < K.
      s = min(max(1, floor(unit * |v| + 0.5)), 32767), the same for every step of a rollout: proportional to the step length.
    Entry (p, t) = (da, db, dk, s); no entry has s <= 0, so every rollout has length T."""
    who = "rollout_arcs"
    rot = _int32_array(who, "rotations", rotations, "[K, 2]", lambda sh: len(sh) == 2 and sh[1] == 2 and 1 <= sh[0] <= _lib.GG_HEADINGS_MAX,
                       f" with 1 <= K <= {_lib.GG_HEADINGS_MAX}")
    _check_integers(who, steps=steps, unit=unit)
    if not 1 <= steps <= _lib.GG_ROLLOUTS_MAX_STEPS:
        raise ValueError(f"{who}: steps lies in [1, {_lib.GG_ROLLOUTS_MAX_STEPS}]")
    if not 1 <= unit <= 32767:
        raise ValueError(f"{who}: unit lies in [1, 32767]")
    v = np.atleast_1d(np.asarray(speeds, dtype=np.float64))
    w = np.atleast_1d(np.asarray(turns, dtype=np.float64))
    if v.ndim != 1 or w.ndim != 1 or v.size < 1 or w.size < 1 or not (np.isfinite(v).all() and np.isfinite(w).all()):
        raise ValueError(f"{who}: speeds and turns are non-empty lists of finite numbers")
    if v.size * w.size > _lib.GG_ROLLOUTS_MAX:
        raise ValueError(f"{who}: more than {_lib.GG_ROLLOUTS_MAX} rollouts")
    if np.abs(v).max() * steps * 16 >= 2 ** 30:
        raise ValueError(f"{who}: a speed is too large")
    vv, ww = [g.reshape(-1, 1) for g in np.meshgrid(v, w, indexing="ij")]       # [P, 1]
    phi = ww * np.arange(1, steps + 1, dtype=np.float64)[None, :]               # [P, T]
    straight = ww == 0.0
    safe = np.where(straight, 1.0, ww)
    a = np.where(straight, vv * np.arange(1, steps + 1, dtype=np.float64)[None, :], vv / safe * np.sin(phi))
    b = np.where(straight, 0.0, vv / safe * (1.0 - np.cos(phi)))
    rha = lambda x: (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)
    angle = np.arctan2(rot[:, 1].astype(np.float64), rot[:, 0].astype(np.float64))
    angle = angle - angle[0]
    apart = np.abs(np.angle(np.exp(1j * (phi[:, :, None] - angle[None, None, :]))))  # [P, T, K] in [0, pi]
    out = np.empty((vv.shape[0], steps, 4), dtype=np.int32)
    out[:, :, 0], out[:, :, 1] = rha(16.0 * a), rha(16.0 * b)
    out[:, :, 2] = np.argmin(apart, axis=2)  # (the first of equal minima)
    out[:, :, 3] = np.clip(np.floor(unit * np.abs(vv) + 0.5), 1, _lib.GG_HEADINGS_MAX_COST).astype(np.int32)
    return out


def heading_moves(rotations, *, step: int = 1, unit: int = 10, turn: int = 0, reverse_pct: int = 0, spin: int = 0):
    """The move table of a car-like vehicle for GroundSegmentation.route_headings (gg_heading_moves): int32 [K, 8, 4], entry m of heading
    k = (da, db, k2, s): from (k, (r, c)) to (k2, (r + da, c + db)) at cost s times the clamped cost of the cell entered; s == 0 marks an
    absent entry.  rotations: rotation_table(angles), int32 [K, 2] with 1 <= K <= 32: the forward axis of heading k is (cq, sq) in
    (row, col).  With d_k = `step` (1 .. 3) cells along that axis, rounded half away from zero per component, and s_k = max(1,
    floor(unit * |d_k|)) (unit in 1 .. 1024): slot 0 goes d_k ahead and keeps the heading, slots 1 and 2 go d_k ahead and end one
    heading to the left (k + 1) and to the right (k - 1) at s_k + turn; slots 3 .. 5 are the same three backwards (-d_k) at
    ceil(cost * reverse_pct / 100), absent with reverse_pct == 0 (otherwise >= 100); slots 6 and 7 turn in place by one heading at `spin`,
    absent with spin == 0 or K == 1.  ValueError for a value outside its range or a cost above 32767.  The defaults are a policy of this
    layer alone (the C call has none)."""
    who = "heading_moves"
    try:
        given = np.asarray(rotations)
        rot = np.ascontiguousarray(given.astype(np.int32))
        exact = given.shape == rot.shape and np.array_equal(given, rot)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"{who}: rotations must be [K, 2] int32: {e}") from None
    if rot.ndim != 2 or rot.shape[1] != 2 or not exact or not 1 <= rot.shape[0] <= _lib.GG_HEADINGS_MAX:
        raise ValueError(f"{who}: rotations are [K, 2] int32 with 1 <= K <= {_lib.GG_HEADINGS_MAX}")
    par = {"step": step, "unit": unit, "turn": turn, "reverse_pct": reverse_pct, "spin": spin}
    for name, v in par.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"{who}: {name} is an int32")
    K = rot.shape[0]
    moves = np.zeros((K, _lib.GG_HEADINGS_MAX_MOVES, 4), dtype=np.int32)
    rc = _lib.load().gg_heading_moves(rot.ctypes.data_as(C.POINTER(C.c_int32)), K, int(step), int(unit), int(turn), int(reverse_pct), int(spin),
                                      moves.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != _lib.GG_OK:
        raise ValueError(f"{who}: step in [1, 3], unit in [1, 1024], turn >= 0, reverse_pct 0 or >= 100, spin >= 0, |rotation word| <= {_lib.GG_MATCH_UNIT} "
                         f"and every cost <= {_lib.GG_HEADINGS_MAX_COST}: gg_heading_moves answered {_lib.STATUS.get(rc, rc)}")
    return moves


def goal_planes(cells, rows: int, cols: int, order: str = "row", device=None):
    """A goal plane per map for GroundSegmentation.route_planes from a list of goal cells, for "route from the robot cell": cells[i] is the
    list of (row, col) goals of map i (an empty list: no goal).  Returns torch.int32 [B, rows, cols] ([B, cols, rows] with order="col"): 0 on
    a goal, -1 elsewhere -- the words of a d_frontier plane."""
    import torch

    if order not in ("row", "col"):
        raise ValueError("goal_planes: order is 'row' or 'col'")
    plane = (rows, cols) if order == "row" else (cols, rows)
    host = torch.full((len(cells),) + plane, -1, dtype=torch.int32)
    for i, goals in enumerate(cells):
        for r, c in goals:
            if not (0 <= int(r) < rows and 0 <= int(c) < cols):
                raise ValueError(f"goal_planes: map {i}: cell {(r, c)} lies outside the map")
            host[(i, int(r), int(c)) if order == "row" else (i, int(c), int(r))] = 0
    return host.to(device) if device is not None else host


class GroundSegmentation:
    """Mirror of groundgrid::GroundSegmentation (include/groundgrid/GroundSegmentation.h:48-71)."""

    def __init__(self):
        self._L = _lib.load()
        self._ctx = None
        self._torch_used = False
        self._async = {}

    # -- GroundSegmentation::init(nodeHandle, dimension, resolution) (src/GroundSegmentation.cpp:37-48)
    def init(self, dimension: float = 120.0, resolution: float = 0.33, *, n_slots: int = 1,
             max_points: int = 150_000, device: int = 0, vertical_point_ang_dist: float = 0.0,
             min_dist_squared: float = 0.0):
        if self._ctx:
            self.close()
        for name, v in (("vertical_point_ang_dist", vertical_point_ang_dist), ("min_dist_squared", min_dist_squared)):
            if not (float(v) >= 0.0) or math.isinf(float(v)):   # (what gg_create answers with GG_ERR_GEOMETRY; zero = the reference's value)
                raise GroundGridError(f"gg_create: {name} = {v!r} must be finite and not negative")
        geom = GGGeometry(float(dimension), float(resolution), float(vertical_point_ang_dist), float(min_dist_squared))
        ctx = C.c_void_p()
        rc = self._L.gg_create(C.byref(geom), int(n_slots), int(max_points), int(device), C.byref(ctx))
        if rc != _lib.GG_OK:
            raise GroundGridError(f"gg_create: {_lib.STATUS.get(rc, rc)}")
        self._ctx = ctx
        self.n_slots = n_slots
        self.max_points = max_points
        self.device = device
        r, c = C.c_int(), C.c_int()
        self._L.gg_get_size(ctx, C.byref(r), C.byref(c))
        self.rows, self.cols = r.value, c.value
        res, lx, ly = C.c_double(), C.c_double(), C.c_double()
        self._L.gg_get_geometry(ctx, C.byref(res), C.byref(lx), C.byref(ly))
        self.resolution, self.length = res.value, (lx.value, ly.value)
        self._maps = [GridMap(self, s) for s in range(n_slots)]
        self._score_ids = None
        return self

    def close(self):
        if self._ctx:
            self._L.gg_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def map(self, slot: int = 0) -> GridMap:
        return self._maps[slot]

    def reset_maps(self, first_slot: int = 0, n_slots: Optional[int] = None, odom_z: float = 0.0, pos=(0.0, 0.0), persistent_only: bool = False,
                   on_torch_stream: bool = False):
        """GroundGrid::initGroundGrid values (src/GroundGrid.cpp:71-75) for a range of map states in one launch; with
        persistent_only just ground / groundpatch, the state that outlives a cloud (a "cold" start).  on_torch_stream: enqueue on
        the current torch stream (where filter_batch runs) instead of the context's own."""
        n = self.n_slots - first_slot if n_slots is None else n_slots
        _check(self._L, self._ctx, self._L.gg_reset_maps(self._ctx, first_slot, n, float(pos[0]), float(pos[1]), C.c_float(odom_z),
                                                          1 if persistent_only else 0, self._stream_arg(on_torch_stream)), "gg_reset_maps")
        for s in range(first_slot, first_slot + n):
            self._maps[s]._pos = (float(pos[0]), float(pos[1]))

    def move_maps(self, odoms, base_to_maps, *, slots=None, first_slot: int = 0, rotation: str = "kdl", on_torch_stream: bool = False,
                  stream=None) -> np.ndarray:
        """GroundGrid::update (src/GroundGrid.cpp:83-147) for many map states in one set of launches: map k (slots[k], or first_slot + k)
        moves to odoms[k] = (x, y) with base_to_maps[k] = (tx, ty, tz, qx, qy, qz, qw), exactly as map(slot).move(...) would.
        on_torch_stream: enqueue on the current torch stream (where filter_batch runs); `stream`: a stream handle of the caller's; by
        default the context's own stream.  Returns the [n, 2] index shifts."""
        od = np.ascontiguousarray(np.asarray(odoms, dtype=np.float64).reshape(-1, 2))
        n = od.shape[0]
        poses = np.asarray(base_to_maps, dtype=np.float64).reshape(n, 7)
        planes = np.empty((n, 4), dtype=np.float64)
        for k in range(n):
            M = transform_from_pose(poses[k], rotation)
            planes[k] = (M[2, 0], M[2, 1], M[2, 2], M[2, 3])
        sl = None
        if slots is not None:
            sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(n))
        h = None  # the context's own stream
        if stream is None and on_torch_stream:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        if stream is not None:
            h = stream if stream else _lib.GG_STREAM_DEFAULT  # (0 = torch's default stream = GG_STREAM_DEFAULT)
        shifts = np.zeros((n, 2), dtype=np.int32)
        P = C.POINTER
        rc = self._L.gg_move_maps(self._ctx, n, sl.ctypes.data_as(P(C.c_int32)) if sl is not None else None, first_slot,
                                  od.ctypes.data_as(P(C.c_double)), planes.ctypes.data_as(P(C.c_double)),
                                  shifts.ctypes.data_as(P(C.c_int32)), C.c_void_p(h) if h is not None else None)
        _check(self._L, self._ctx, rc, "gg_move_maps")
        for k in range(n):
            slot = int(sl[k]) if sl is not None else first_slot + k
            x, y = C.c_double(), C.c_double()
            self._L.gg_get_map_position(self._ctx, slot, C.byref(x), C.byref(y))
            self._maps[slot]._pos = (x.value, y.value)
        return shifts

    def export_layers(self, names=None, *, slots=None, first_slot: int = 0, n: Optional[int] = None, out=None, row_major: bool = False,
                      stream=None, own_stream: bool = False, plane_stride: Optional[int] = None):
        """The named layers (default: all eleven, in gg_layer order) of many maps as one CUDA torch.float32 tensor [n, K, cols, rows]
        (Eigen's column-major planes: element [i, k, c, r] is cell (r, c)), or [n, K, rows, cols] with row_major -- what
        map(slot).layers() returns for each map, bit for bit, without leaving the device (gg_export_layers).  Map i = slots[i], or
        first_slot + i for n maps (default: up to the last slot).  `out` (same shape, contiguous) is reused when given.  Enqueued on the
        current torch stream like filter_batch (or on `stream`), without synchronising: torch ops enqueued there afterwards see the
        planes.  Fresh maps stay fresh; the three lazily kept layers are computed first where the mask names them.
        own_stream: enqueue on the context's own stream instead (the caller orders its own streams around the call).  plane_stride
        (in floats, >= rows * cols): the planes lie that far apart in a flat [n * K * plane_stride] tensor, which is returned (or `out`
        of that size reused); the elements between a plane's end and the next plane are not written."""
        return self._transfer("export_layers", names, _LAYER_NAMES, out, slots, first_slot, n, row_major, stream, own_stream, plane_stride)

    def _transfer(self, who, names, known, planes, slots, first_slot, n, row_major, stream, own_stream, plane_stride):
        """export_layers, export_slopes and import_layers (`who`): the names of `known` (_name_mask's arguments) to their mask, the shape of
        the three forms, `planes` checked -- the `out` of an export, made when there is none; the source of the import --, the call."""
        import torch

        self._torch_used = True
        names, mask = _name_mask(who, known[0] if names is None else names, *known)
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        shape = (cnt, len(names), self.rows, self.cols) if row_major else (cnt, len(names), self.cols, self.rows)
        if plane_stride is not None:
            shape = (cnt * len(names) * int(plane_stride),)
        if who == "import_layers":
            if not (torch.is_tensor(planes) and planes.is_cuda and planes.dtype == torch.float32 and planes.is_contiguous()):
                raise ValueError(f"{who}: planes must be a contiguous CUDA float32 tensor")
            if tuple(planes.shape) != shape:
                raise ValueError(f"{who}: planes has shape {tuple(planes.shape)}, these arguments need {shape}")
        elif planes is None:
            planes = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", self.device))
        elif not _is_dense(planes, shape, torch.float32):
            raise ValueError(f"{who}: out must be a contiguous CUDA float32 tensor of shape {shape}")
        rc = getattr(self._L, "gg_" + who)(self._ctx, cnt, ptr, first, mask, _lib.GG_PLANES_ROWMAJOR if row_major else _lib.GG_PLANES_COLMAJOR,
                                           C.c_void_p(planes.data_ptr()), self.rows * self.cols if plane_stride is None else int(plane_stride),
                                           self._stream_arg(not own_stream, handle=stream))
        _check(self._L, self._ctx, rc, "gg_" + who)
        return planes

    def export_slopes(self, names=None, *, slots=None, first_slot: int = 0, n: Optional[int] = None, out=None, row_major: bool = False,
                      stream=None, own_stream: bool = False, plane_stride: Optional[int] = None):
        """The shape of the terrain of many maps (gg_export_slopes): the named channels of _lib.SLOPE_CHANNELS (default: all six; distinct
        and in that order) as one CUDA torch.float32 tensor with the shapes of export_layers -- [n, K, cols, rows] (element [i, k, c, r] is
        cell (r, c)), [n, K, rows, cols] with row_major, or the flat [n * K * plane_stride] tensor.  grad_x / grad_y are dz/dx and dz/dy in
        the map frame (rows grow towards -x, columns towards -y; central differences, one-sided on the border), tangent and normal_z the
        tangent and the cosine of the slope angle, step the largest height difference to one of the up to eight neighbours,
        min_confidence the smallest groundpatch value of the cell and its neighbours; include/groundgrid_hip.h defines them to the bit.
        Computed from the maps' ground / groundpatch layers as they stand, in one launch, without synchronising; nothing of a map
        changes, fresh maps stay fresh and the lazily kept layers stay pending.  Map selection, `out`, `stream`, `own_stream` and
        `plane_stride` are those of export_layers."""
        return self._transfer("export_slopes", names, _SLOPE_NAMES, out, slots, first_slot, n, row_major, stream, own_stream, plane_stride)

    def import_layers(self, planes, names=None, *, slots=None, first_slot: int = 0, n: Optional[int] = None, row_major: bool = False,
                      stream=None, own_stream: bool = False, plane_stride: Optional[int] = None):
        """The inverse of export_layers (gg_import_layers): `planes`, a contiguous CUDA torch.float32 tensor of exactly the shape
        export_layers returns for the same arguments ([n, K, cols, rows], [n, K, rows, cols] with row_major, or the flat
        [n * K * plane_stride] tensor), becomes the named layers (default: all eleven, in gg_layer order) of the maps -- bit for bit what
        map(slot).set(name, plane) would leave for every one of them, without a host round trip.  Layers that are not named keep their
        values; positions, configurations and scores are untouched.  Enqueued on the current torch stream (or on `stream`) without
        synchronising: `planes` must stay unmodified until that stream has passed the call, which torch ops enqueued there afterwards
        do by themselves.  own_stream: on the context's own stream instead (the caller orders its own streams around the call)."""
        self._transfer("import_layers", names, _LAYER_NAMES, planes, slots, first_slot, n, row_major, stream, own_stream, plane_stride)

    def export_images(self, names=None, *, terrain: bool = False, chw: bool = False, slots=None, first_slot: int = 0, n: Optional[int] = None,
                      out=None, on_torch_stream: bool = False) -> ImageExport:
        """The 8-bit images of the named layers (default: all eleven, in gg_layer order; [] for none) and, with terrain, the 32FC3
        terrain images of many maps as CUDA torch tensors (gg_export_images): images uint8 [n, K, rows, cols] and bounds float32
        [n, K, 2] -- per map and layer what map(slot).image_u8(name) returns, byte for byte --, terrain float32 [n, rows, cols, 3] --
        map(slot).terrain_image() bit for bit -- or [n, 3, rows, cols] with chw.  Map i = slots[i], or first_slot + i for n maps
        (default: up to the last slot).  `out`: an ImageExport of an earlier call with the same arguments, whose tensors are reused.
        Enqueued without synchronising, on the context's own stream (torch.cuda.synchronize() before torch reads the tensors; synchronize() fills the fresh maps) or, with
        on_torch_stream, on the current torch stream, where torch ops enqueued afterwards see them.  Fresh maps stay fresh; the three
        lazily kept layers are computed first where the names ask for one."""
        import torch

        self._torch_used = True
        names, mask = _name_mask("export_images", LAYERS if names is None else names, *_LAYER_NAMES)
        if not names and not terrain:
            raise ValueError("export_images: neither a layer nor the terrain image is asked for")
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        K = len(names)
        want = {"images": ((cnt, K, self.rows, self.cols), torch.uint8) if K else None, "bounds": ((cnt, K, 2), torch.float32) if K else None,
                "terrain": ((cnt, 3, self.rows, self.cols) if chw else (cnt, self.rows, self.cols, 3), torch.float32) if terrain else None}
        res = _reuse_outputs("export_images", out if out is not None else ImageExport(), want, torch.device("cuda", self.device))
        x = _lib.GGImageExport()
        x.n, x.first_slot, x.slots, x.layer_mask = cnt, first, ptr, mask
        x.d_images = res.images.data_ptr() if K else None
        x.image_stride = self.rows * self.cols
        x.d_bounds = res.bounds.data_ptr() if K else None
        x.d_terrain = res.terrain.data_ptr() if terrain else None
        x.terrain_stride = 3 * self.rows * self.cols
        x.terrain_layout = _lib.GG_TERRAIN_CHW if chw else _lib.GG_TERRAIN_HWC
        stream = self._stream_arg(on_torch_stream)
        _check(self._L, self._ctx, self._L.gg_export_images(self._ctx, C.byref(x), stream), "gg_export_images")
        return res

    def split_clouds(self, points, n_points: Sequence[int], *, labels=None, masks=None, transforms=None, slots=None, first_slot: int = 0,
                     ground: bool = True, nonground: bool = True, heights: bool = True, sources: bool = True, out: Optional[SplitOutputs] = None,
                     on_torch_stream: bool = True) -> SplitOutputs:
        """The ground (label 49) and the non-ground (label 99) points of many labelled clouds as dense clouds on the device
        (gg_split_clouds): per set the packed 16-byte records uint8 [B, stride, 16] in the map frame, float32 [B, stride] heights above the
        map's `ground` layer as it stands, int32 [B, stride] indices into the input cloud, and counts int32 [B, 2] -- in the cloud's own
        order, what points[b][labels[b] == 99] gives, without a synchronisation: the sizes stay on the device (SplitOutputs.clouds() reads
        them).  points / n_points / transforms / slots / first_slot as for filter_batch; exactly one of labels (uint8 [B, stride], BatchOutputs.labels)
        and masks (uint8 [B, stride // 4], BatchOutputs.label_masks).  ground / nonground: which sets are written; heights / sources:
        whether their height and source tensors are.  `out`: a SplitOutputs of an earlier call with the same arguments, whose tensors are
        reused.  Enqueued on the current torch stream (where filter_batch runs and torch ops enqueued afterwards see the outputs) or, with
        on_torch_stream=False, on the context's own stream.  No map changes; fresh maps stay fresh."""
        import torch

        self._torch_used = True
        x = _lib.GGCloudSplit()
        B, stride, keep = self._labelled_clouds("split_clouds", x, points, n_points, labels, masks, transforms, slots, first_slot)
        want = {"counts": (B, 2)}
        for name, on in (("ground", ground), ("nonground", nonground)):
            want[f"{name}_points"] = ((B, stride, 16), torch.uint8) if on else None
            want[f"{name}_height"] = ((B, stride), torch.float32) if on and heights else None
            want[f"{name}_source"] = (B, stride) if on and sources else None
        res = _reuse_outputs("split_clouds", out if out is not None else SplitOutputs(), want, points.device)
        for name, dst in (("ground", x.ground), ("nonground", x.nonground)):
            for k in ("points", "height", "source"):
                t = getattr(res, f"{name}_{k}")
                setattr(dst, f"d_{k}", t.data_ptr() if t is not None else None)
        x.d_counts = res.counts.data_ptr()
        stream = self._stream_arg(on_torch_stream, points.device)
        _check(self._L, self._ctx, self._L.gg_split_clouds(self._ctx, C.byref(x), stream), "gg_split_clouds")
        return res

    def rasterize_clouds(self, points, n_points: Sequence[int], *, labels=None, masks=None, transforms=None, slots=None, first_slot: int = 0,
                         channels: Sequence[str] = ("nonground_count", "nonground_max_height"), order: str = "row", out=None,
                         on_torch_stream: bool = True):
        """The obstacle grid of many labelled clouds on the device (gg_rasterize_clouds): a CUDA torch.float32 tensor [B, K, rows, cols]
        (order="row"; [B, K, cols, rows], Eigen's column-major planes, with order="col" -- the shapes of export_layers) whose plane k is the
        k-th of `channels`: per cell of cloud b's map the number of its non-ground (label 99) / ground (label 49) points there as a float
        ("nonground_count", "ground_count"), and the largest and the smallest height of them above the map's `ground` layer as it stands
        ("..._max_height", "..._min_height"; NaN where the cell holds no such point).  channels: distinct names of _lib.RASTER_CHANNELS in
        that order.  points / n_points / transforms / slots / first_slot and labels / masks as for split_clouds.  `out` (same shape,
        contiguous) is reused and returned when given.  Independent of the order in which points arrive: bit-identical from run to run.
        Enqueued on the current torch stream (where filter_batch runs and torch ops enqueued afterwards see the planes) or, with
        on_torch_stream=False, on the context's own stream.  No map changes; fresh maps stay fresh."""
        import torch

        self._torch_used = True
        x = _lib.GGCloudRaster()
        B, stride, keep = self._labelled_clouds("rasterize_clouds", x, points, n_points, labels, masks, transforms, slots, first_slot)
        channels, x.channel_mask = _name_mask("rasterize_clouds", channels, _lib.RASTER_CHANNELS, "channels must be distinct, in GG_RASTER_* order, and at least one",
                                              "channels")
        plane, x.order = _plane_order("rasterize_clouds", order, self.rows, self.cols)
        shape = (B, len(channels)) + plane
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=points.device)
        elif not _is_dense(out, shape, torch.float32):
            raise ValueError(f"rasterize_clouds: out must be a contiguous CUDA float32 tensor of shape {shape}")
        x.d_dst, x.plane_stride = out.data_ptr(), self.rows * self.cols
        stream = self._stream_arg(on_torch_stream, points.device)
        _check(self._L, self._ctx, self._L.gg_rasterize_clouds(self._ctx, C.byref(x), stream), "gg_rasterize_clouds")
        return out

    def cluster_clouds(self, points, n_points: Sequence[int], *, labels=None, masks=None, transforms=None, slots=None, first_slot: int = 0,
                       min_points: int = 1, min_height: float = -math.inf, max_height: float = math.inf, connectivity: int = 8,
                       max_clusters: int = 256, order: str = "row", point_clusters: bool = True, out: Optional[ClusterOutputs] = None,
                       on_torch_stream: bool = True) -> ClusterOutputs:
        """The obstacle clusters of many labelled clouds on the device (gg_cluster_clouds): the connected components (connectivity 4 or 8)
        of the cells that hold at least min_points non-ground (label 99) points whose height above the map's `ground` layer as it stands
        lies in [min_height, max_height].  ClusterOutputs: cell_cluster int32 [B, rows, cols] (order="row"; [B, cols, rows] with
        order="col") with -1 or the cell's cluster id, the clusters of a map numbered by their smallest linear cell index of `order` (with
        "row": scipy.ndimage.label(occupied)[0] - 1); n_clusters int32 [B], the true counts; clusters int32 [B, max_clusters, 8], the
        gg_cluster records of the first max_clusters clusters (None with max_clusters=0; ClusterOutputs.table(b) reads them as a numpy
        structured array); point_cluster int32 [B, stride], the id of every point's cell or -1 (None with point_clusters=False; elements
        behind n_points[b] are not written).  points / n_points / transforms / slots / first_slot and labels / masks as for
        rasterize_clouds.  `out`: a ClusterOutputs of an earlier call with the same arguments, whose tensors are reused.  Only integer
        atomics: bit-identical from run to run.  Enqueued on the current torch stream or, with on_torch_stream=False, on the context's own
        stream; nothing synchronises.  No map changes; fresh maps stay fresh."""
        self._torch_used = True
        x = _lib.GGCloudClusters()
        B, stride, keep = self._labelled_clouds("cluster_clouds", x, points, n_points, labels, masks, transforms, slots, first_slot)
        if connectivity not in (4, 8):
            raise ValueError("cluster_clouds: connectivity is 4 or 8")
        plane, x.order = _plane_order("cluster_clouds", order, self.rows, self.cols)
        max_clusters = int(max_clusters)
        if max_clusters < 0:
            raise ValueError("cluster_clouds: max_clusters < 0")
        want = {"cell_cluster": (B,) + plane, "n_clusters": (B,), "clusters": (B, max_clusters, 8) if max_clusters else None,
                "point_cluster": (B, stride) if point_clusters else None}
        res = _reuse_outputs("cluster_clouds", out if out is not None else ClusterOutputs(), want, points.device)
        x.min_points, x.min_height, x.max_height, x.connectivity = int(min_points), float(min_height), float(max_height), int(connectivity)
        x.d_cell_cluster, x.plane_stride = res.cell_cluster.data_ptr(), self.rows * self.cols
        x.d_point_cluster = res.point_cluster.data_ptr() if point_clusters else None
        x.d_n_clusters = res.n_clusters.data_ptr()
        x.d_clusters = res.clusters.data_ptr() if max_clusters else None
        x.max_clusters = max_clusters
        stream = self._stream_arg(on_torch_stream, points.device)
        _check(self._L, self._ctx, self._L.gg_cluster_clouds(self._ctx, C.byref(x), stream), "gg_cluster_clouds")
        return res

    def _clearance_call(self, who, x, B, device, max_cells, plane, nearest, distance, out, on_torch_stream):
        """What clearance_clouds and clearance_planes (`who`) share: the outputs of B maps on `device`, the rest of `x`, the call."""
        import torch

        want = {"dist2": (B,) + plane, "nearest": (B,) + plane if nearest else None,
                "distance": ((B,) + plane, torch.float32) if distance else None, "n_occupied": (B,)}
        res = _reuse_outputs(who, out if out is not None else ClearanceOutputs(), want, device)
        x.max_cells = max_cells
        x.d_dist2, x.plane_stride = res.dist2.data_ptr(), self.rows * self.cols
        x.d_nearest = res.nearest.data_ptr() if nearest else None
        x.d_distance = res.distance.data_ptr() if distance else None
        x.d_n_occupied = res.n_occupied.data_ptr()
        stream = self._stream_arg(on_torch_stream, device)
        _check(self._L, self._ctx, self._L.gg_clearance_clouds(self._ctx, C.byref(x), stream), "gg_clearance_clouds")
        return res

    def clearance_clouds(self, points, n_points: Sequence[int], *, labels=None, masks=None, transforms=None, slots=None, first_slot: int = 0,
                         min_points: int = 1, min_height: float = -math.inf, max_height: float = math.inf, max_cells: int = 0,
                         order: str = "row", nearest: bool = True, distance: bool = True, out: Optional[ClearanceOutputs] = None,
                         on_torch_stream: bool = True) -> ClearanceOutputs:
        """The obstacle distance field of many labelled clouds on the device (gg_clearance_clouds, cloud mode): per cell of cloud b's map
        the exact squared Euclidean distance, in cells, to the nearest occupied cell (dist2, 0 on an occupied cell), the linear index of
        that cell in `order` (nearest; of several equally near ones the smallest row, then the smallest column) and the distance in metres
        (distance = sqrt(dist2) * resolution).  A cell is occupied exactly where cluster_clouds with the same points, labels / masks,
        transforms, slots, min_points, min_height and max_height gives cell_cluster >= 0.  max_cells=R > 0 reports no obstacle beyond R
        cells.  No obstacle: dist2 = _lib.GG_CLEARANCE_NONE, nearest = -1, distance = +inf.  n_occupied int32 [B] counts the occupied cells.
        nearest=False / distance=False leave those planes out (None).  `out`: a ClearanceOutputs of an earlier call with the same
        arguments, whose tensors are reused.  Integer arithmetic only: bit-identical from run to run.  Enqueued on the current torch
        stream or, with on_torch_stream=False, on the context's own stream; nothing synchronises.  No map changes; fresh maps stay fresh."""
        who = "clearance_clouds"
        x = _lib.GGCloudClearance()
        plane, x.order = _plane_order(who, order, self.rows, self.cols)
        max_cells = _max_cells(who, max_cells)
        x.min_points, x.min_height, x.max_height = _occupancy(who, min_points, min_height, max_height)
        self._torch_used = True
        B, stride, keep = self._labelled_clouds(who, x, points, n_points, labels, masks, transforms, slots, first_slot)
        return self._clearance_call(who, x, B, points.device, max_cells, plane, nearest, distance, out, on_torch_stream)

    def clearance_planes(self, seeds, *, max_cells: int = 0, order: str = "row", nearest: bool = True, distance: bool = True,
                         out: Optional[ClearanceOutputs] = None, on_torch_stream: bool = True) -> ClearanceOutputs:
        """The obstacle distance field of occupancy planes the caller holds (gg_clearance_clouds, seed mode): seeds is a contiguous CUDA
        torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"), B <= n_slots, whose cells are occupied where the word is
        >= 0 -- ClusterOutputs.cell_cluster as it is, or any plane thresholded into {-1, 0}.  Everything else as clearance_clouds; no map
        is read.  seeds may not be one of the outputs."""
        import torch

        who = "clearance_planes"
        x = _lib.GGCloudClearance()
        plane, x.order = _plane_order(who, order, self.rows, self.cols)
        max_cells = _max_cells(who, max_cells)
        if not (torch.is_tensor(seeds) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.dim() == 3 and seeds.is_contiguous()):
            raise ValueError(f"{who}: seeds must be a contiguous CUDA torch.int32 tensor [B, rows, cols]")
        B = int(seeds.shape[0])
        if tuple(seeds.shape[1:]) != plane:
            raise ValueError(f"{who}: seeds of shape {tuple(seeds.shape)} do not fit planes of {plane}")
        if out is not None and out.dist2 is not None and torch.is_tensor(out.dist2) and out.dist2.data_ptr() == seeds.data_ptr():
            raise ValueError(f"{who}: seeds may not be an output")
        self._torch_used = True
        x.n, x.d_seeds, x.seed_stride = B, seeds.data_ptr(), self.rows * self.cols
        return self._clearance_call(who, x, B, seeds.device, max_cells, plane, nearest, distance, out, on_torch_stream)

    def visibility_clouds(self, points, n_points: Sequence[int], origins, *, labels=None, masks=None, transforms=None, slots=None,
                          first_slot: int = 0, min_points: int = 1, min_height: float = -math.inf, max_height: float = math.inf,
                          max_cells: int = 0, order: str = "row", counts: bool = True, out: Optional[VisibilityOutputs] = None,
                          on_torch_stream: bool = True) -> VisibilityOutputs:
        """Where the sensor saw what, for many labelled clouds on the device (gg_visibility_clouds): state int32 [B, rows, cols]
        (order="row"; [B, cols, rows] with order="col") holds _lib.GG_CELL_OCCUPIED (1) exactly where cluster_clouds with the same points,
        labels / masks, transforms, slots, min_points, min_height and max_height gives cell_cluster >= 0; else _lib.GG_CELL_FREE (-1) where
        a ground or non-ground return (label 49 / 99) landed or the integer ray from the sensor cell to the cell of such a return passed;
        else _lib.GG_CELL_UNKNOWN (0).  origins: [B, 3] float32 (anything np.asarray turns into that), the sensor in the MAP frame as for
        filter_batch; only x and y are used, and a sensor outside its map or not finite casts no ray.  One ray per distinct cell with a
        return; an occupied cell does not stop it; max_cells=R > 0 clears at most the first R cells of a ray.  Returns outside the map
        clear nothing inside it.  counts int32 [B, 3]: the free, unknown and occupied cells of every map (None with counts=False).  A state
        plane is a seed plane of clearance_planes as it stands (cells >= 0: occupied or never observed).  `out`: a VisibilityOutputs of
        an earlier call with the same arguments, whose tensors are reused.  Integer arithmetic only: bit-identical from run to run.
        Enqueued on the current torch stream or, with on_torch_stream=False, on the context's own stream; nothing synchronises.  No map
        changes; fresh maps stay fresh."""
        import torch

        who = "visibility_clouds"
        x = _lib.GGCloudVisibility()
        plane, x.order = _plane_order(who, order, self.rows, self.cols)
        x.max_cells = _max_cells(who, max_cells)
        x.min_points, x.min_height, x.max_height = _occupancy(who, min_points, min_height, max_height)
        try:
            host_origins = np.ascontiguousarray(np.asarray(origins, dtype=np.float32))
        except (TypeError, ValueError) as e:
            raise ValueError(f"{who}: origins must be [B, 3] float32: {e}") from None
        if host_origins.ndim != 2 or host_origins.shape[1] != 3 or not torch.is_tensor(points) or host_origins.shape[0] != points.shape[0]:
            raise ValueError(f"{who}: origins of shape {host_origins.shape} are not [B, 3]")
        self._torch_used = True
        B, stride, keep = self._labelled_clouds(who, x, points, n_points, labels, masks, transforms, slots, first_slot)
        want = {"state": (B,) + plane, "counts": (B, 3) if counts else None}
        res = _reuse_outputs(who, out if out is not None else VisibilityOutputs(), want, points.device)
        x.origins = host_origins.ctypes.data_as(C.POINTER(C.c_float))
        x.d_state, x.plane_stride = res.state.data_ptr(), self.rows * self.cols
        x.d_counts = res.counts.data_ptr() if counts else None
        stream = self._stream_arg(on_torch_stream, points.device)
        _check(self._L, self._ctx, self._L.gg_visibility_clouds(self._ctx, C.byref(x), stream), "gg_visibility_clouds")
        return res

    def fuse_states(self, states, evidence=None, *, shifts=None, hit: int = 4, miss: int = 1, decay: int = 0, e_min: int = -16,
                    e_max: int = 32, free_threshold: int = -2, occ_threshold: int = 4, order: str = "row", fused: bool = True,
                    frontier: bool = True, counts: bool = True, out: Optional[FusionOutputs] = None,
                    on_torch_stream: bool = False) -> FusionOutputs:
        """The occupancy grid that persists across scans (gg_fuse_states).  states: a contiguous CUDA torch.int32 tensor [B, rows, cols]
        ([B, cols, rows] with order="col"), B <= n_slots, this scan's observation -- VisibilityOutputs.state as it is: > 0 occupied, < 0
        free, 0 not observed.  evidence: FusionOutputs.evidence of the previous call (same shape), or None for no prior.  shifts: what
        move_maps returned for the move between the two scans, [B, 2] (anything np.asarray turns into int32 of that shape), or None for
        no move; a cell the move exposed starts without evidence.  Per cell, in integers: the prior is clamped to [e_min, e_max] and moves
        `decay` towards 0; an occupied observation adds `hit`, a free one subtracts `miss`; the clamped sum is the new evidence.  state is
        OCCUPIED from occ_threshold up, FREE from free_threshold down, UNKNOWN between; frontier is 0 on a FREE cell with an UNKNOWN one
        among its eight neighbours and -1 elsewhere; counts int32 [B, 4]: free, unknown, occupied, frontier cells.  The defaults are a
        policy of this layer alone (the C call has none): one hit marks a cell, two misses free an unknown one, and a cell hit once is
        unknown again after one miss.
        state and frontier are seed planes of clearance_planes as they stand.  fused=False / frontier=False / counts=False leave those
        out (None).  `out`: a FusionOutputs of an earlier call with the same arguments, whose tensors are reused; it may not hold
        `evidence` or `states` -- no update in place is defined, alternate between two FusionOutputs.  Integer arithmetic only:
        bit-identical from run to run.  Enqueued on the context's own stream or, with on_torch_stream=True, on the current torch stream;
        nothing synchronises.  No map is read or changed."""
        who = "fuse_states"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, hit=hit, miss=miss, decay=decay, e_min=e_min, e_max=e_max, free_threshold=free_threshold, occ_threshold=occ_threshold)
        lim = _lib.GG_FUSE_LIMIT
        if not (0 <= hit <= lim and 0 <= miss <= lim and 0 <= decay <= lim):
            raise ValueError(f"{who}: hit, miss and decay lie in [0, 2^30 - 1]")
        if not (-lim <= e_min <= 0 <= e_max <= lim):
            raise ValueError(f"{who}: -(2^30 - 1) <= e_min <= 0 <= e_max <= 2^30 - 1")
        if not (e_min <= free_threshold <= -1 and 1 <= occ_threshold <= e_max):
            raise ValueError(f"{who}: e_min <= free_threshold <= -1 and 1 <= occ_threshold <= e_max")
        if not _is_planes(states, plane):
            raise ValueError(f"{who}: states must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(states.shape[0])
        if evidence is not None and not (_is_planes(evidence, plane) and evidence.shape[0] == B and evidence.device == states.device):
            raise ValueError(f"{who}: evidence must be a contiguous CUDA torch.int32 tensor of the shape and device of states")
        host_shifts = _int32_array(who, "shifts", shifts, "[B, 2]", lambda sh: sh == (B, 2)) if shifts is not None else None
        shape = (B,) + plane
        want = {"evidence": shape, "state": shape if fused else None, "frontier": shape if frontier else None, "counts": (B, 4) if counts else None}
        res = _reuse_outputs(who, out if out is not None else FusionOutputs(), want, states.device, [t.data_ptr() for t in (states, evidence) if t is not None])
        self._torch_used = True
        x = _lib.GGStateFusion()
        x.n, x.d_state, x.state_stride = B, states.data_ptr(), self.rows * self.cols
        x.d_evidence_in = evidence.data_ptr() if evidence is not None else None
        if host_shifts is not None:
            x.shifts = _int32_ptr(host_shifts)
        x.hit, x.miss, x.decay, x.e_min, x.e_max = int(hit), int(miss), int(decay), int(e_min), int(e_max)
        x.free_threshold, x.occ_threshold = int(free_threshold), int(occ_threshold)
        x.order = c_order
        x.d_evidence_out, x.plane_stride = res.evidence.data_ptr(), self.rows * self.cols
        x.d_fused = res.state.data_ptr() if fused else None
        x.d_frontier = res.frontier.data_ptr() if frontier else None
        x.d_counts = res.counts.data_ptr() if counts else None
        stream = self._stream_arg(on_torch_stream, states.device)
        _check(self._L, self._ctx, self._L.gg_fuse_states(self._ctx, C.byref(x), stream), "gg_fuse_states")
        return res

    def route_planes(self, goals, blocked=None, cost=None, *, connectivity: int = 8, straight: int = 5, diagonal: int = 7, cost_max: int = 252,
                     max_cost: int = 0, order: str = "row", next: bool = True, counts: bool = True, starts=None, max_path: int = 0,
                     out: Optional[RouteOutputs] = None, on_torch_stream: bool = False) -> RouteOutputs:
        """The navigation function of many maps (gg_route_planes): per cell the exact cost of the cheapest admissible path to the nearest goal
        cell, and the next cell on it.  goals: a contiguous CUDA torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"),
        B <= n_slots: a goal where the word is >= 0 and the cell is not blocked -- FusionOutputs.frontier as it is, or goal_planes() of a list
        of cells.  blocked: same shape or None: blocked where the word is >= 0 -- FusionOutputs.state as it is (occupied or never observed).
        cost: same shape or None: a step INTO a cell costs straight (diagonal) * min(max(word, 1), cost_max); None: 1 everywhere.  A diagonal
        step also needs both side cells unblocked.  dist is _lib.GG_ROUTE_NONE where no path leads to a goal, or where it costs more than
        max_cost > 0.  next: own index on a goal, -1 on an unreached cell, else the first neighbour, in the order N, W, E, S, NW, NE, SW, SE of
        (row, col), that attains the minimum.  counts int32 [B, 3]: goals, reached, unblocked cells.
        starts: [B] linear cell indices in `order` (anything np.asarray turns into int32), -1 for no start: with max_path >= 1, paths
        [B, max_path] holds start, next(start), ... up to the goal and path_len [B] the length of the whole path (0: unreached); the words of
        paths from path_len on keep what they held (they are -1 in a tensor this call allocates).
        The limit max(straight, diagonal) * cost_max * rows * cols <= 2^31 - 2 keeps every sum inside an int32.  The defaults (5, 7, 252) are
        a policy of this layer alone (the C call has none).  next=False / counts=False leave those out (None).  `out`: a RouteOutputs of an
        earlier call with the same arguments, whose tensors are reused; it may not hold an input.  Integer arithmetic only: bit-identical
        from run to run.  Enqueued on the context's own stream or, with on_torch_stream=True, on the current torch stream; nothing
        synchronises.  No map is read or changed."""
        who = "route_planes"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, connectivity=connectivity, straight=straight, diagonal=diagonal, cost_max=cost_max, max_cost=max_cost, max_path=max_path)
        if connectivity not in (4, 8):
            raise ValueError(f"{who}: connectivity is 4 or 8")
        if not (1 <= straight <= 65535 and (connectivity == 4 or 1 <= diagonal <= 65535)):
            raise ValueError(f"{who}: straight and diagonal lie in [1, 65535]")
        if cost_max < 1:
            raise ValueError(f"{who}: cost_max >= 1")
        if not 0 <= max_cost <= _lib.GG_ROUTE_NONE:
            raise ValueError(f"{who}: max_cost lies in [0, 2^31 - 1]")
        if max_path < 0 or (starts is None and max_path != 0):
            raise ValueError(f"{who}: max_path is >= 1 with starts and 0 without")
        if max(straight, diagonal if connectivity == 8 else 0) * cost_max * self.rows * self.cols > _lib.GG_ROUTE_LIMIT:
            raise ValueError(f"{who}: max(straight, diagonal) * cost_max * rows * cols exceeds 2^31 - 2")
        if not _is_planes(goals, plane):
            raise ValueError(f"{who}: goals must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(goals.shape[0])
        for name, t in (("blocked", blocked), ("cost", cost)):
            if t is not None and not (_is_planes(t, plane) and t.shape[0] == B and t.device == goals.device):
                raise ValueError(f"{who}: {name} must be a contiguous CUDA torch.int32 tensor of the shape and device of goals")
        host_starts = None
        if starts is not None:
            host_starts = _int32_array(who, "starts", starts, "[B]", lambda sh: sh == (B,))
            if ((host_starts < -1) | (host_starts >= self.rows * self.cols)).any():
                raise ValueError(f"{who}: a start lies outside [-1, rows * cols)")
            if max_path < 1:
                raise ValueError(f"{who}: starts needs max_path >= 1")
        shape = (B,) + plane
        with_paths = host_starts is not None
        want = {"dist": shape, "next": shape if next else None, "counts": (B, 3) if counts else None,
                "paths": (B, max_path) if with_paths else None, "path_len": (B,) if with_paths else None}
        # (the call leaves the words behind a path alone: -1 in a tensor allocated here)
        res = _reuse_outputs(who, out if out is not None else RouteOutputs(), want, goals.device, [t.data_ptr() for t in (goals, blocked, cost) if t is not None],
                             fill={"paths": -1})
        self._torch_used = True
        x = _lib.GGPlaneRoutes()
        cells = self.rows * self.cols
        x.n, x.d_goals, x.goal_stride = B, goals.data_ptr(), cells
        x.d_blocked, x.blocked_stride = (blocked.data_ptr(), cells) if blocked is not None else (None, 0)
        x.d_cost, x.cost_stride = (cost.data_ptr(), cells) if cost is not None else (None, 0)
        x.connectivity, x.straight, x.diagonal, x.cost_max, x.max_cost = int(connectivity), int(straight), int(diagonal), int(cost_max), int(max_cost)
        x.order = c_order
        x.d_dist, x.plane_stride = res.dist.data_ptr(), cells
        x.d_next = res.next.data_ptr() if next else None
        x.d_counts = res.counts.data_ptr() if counts else None
        if with_paths:
            x.starts = _int32_ptr(host_starts)
            x.d_paths, x.max_path, x.d_path_len = res.paths.data_ptr(), int(max_path), res.path_len.data_ptr()
        stream = self._stream_arg(on_torch_stream, goals.device)
        _check(self._L, self._ctx, self._L.gg_route_planes(self._ctx, C.byref(x), stream), "gg_route_planes")
        return res

    def match_planes(self, scan, field, *, shifts=None, pivots=None, rotations=None, window: int = 8, field_max: int = 32, order: str = "row",
                     scores: bool = False, out: Optional[MatchOutputs] = None, on_torch_stream: bool = False) -> MatchOutputs:
        """Correlative scan-to-map matching of many maps (gg_match_planes): which yaw candidate and which translation of a window lay this
        scan's occupied cells best over the accumulated grid.  scan: a contiguous CUDA torch.int32 tensor [B, rows, cols] ([B, cols, rows]
        with order="col"), B <= n_slots: a scan cell where the word is > 0 -- VisibilityOutputs.state or FusionOutputs.state as it is.
        field: same shape: a cell's reward is min(max(word, 0), field_max), 0 outside the map -- FusionOutputs.evidence of the previous
        call as it is.  shifts: the prior shift per map, [B, 2] with the meaning it has in fuse_states (scan cell (r, c) lies over field
        cell (r + s0, c + s1)), or None for no move.  pivots: the centre of rotation per map, [B, 2] (row, col) inside the map, or None for
        (rows // 2, cols // 2).  rotations: rotation_table(angles), int32 [K, 2] with 1 <= K <= 64 and |word| <= 16384, or None for the
        identity alone.  window: W in [0, 32]: the translations (dy, dx) in [-W, W]^2.
        best int32 [B, 6]: k*, dy*, dx*, the best score S*, the scan cells of the map, and how many candidates attain S*; among equal
        scores the smallest dy^2 + dx^2 wins, then the smallest k, dy, dx.  With k* the identity, shifts[i] + (dy*, dx*) is the corrected
        shift to hand to fuse_states; another k* is a yaw correction for the next cloud-to-map transform.  scores=True adds the volumes,
        int32 [B, K, 2 W + 1, 2 W + 1].  The limit field_max * rows * cols <= 2^31 - 1 keeps every score inside an int32; the default
        field_max is the default e_max of fuse_states, a policy of this layer alone (the C call has none).  `out`: a MatchOutputs of an
        earlier call with the same arguments, whose tensors are reused; it may not hold an input.  Integer sums only: bit-identical from
        run to run.  Enqueued on the context's own stream or, with on_torch_stream=True, on the current torch stream; nothing
        synchronises.  No map is read or changed."""
        who = "match_planes"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, window=window, field_max=field_max)
        if not 0 <= window <= _lib.GG_MATCH_MAX_WINDOW:
            raise ValueError(f"{who}: window lies in [0, {_lib.GG_MATCH_MAX_WINDOW}]")
        if field_max < 1 or field_max * self.rows * self.cols > _lib.GG_MATCH_LIMIT:
            raise ValueError(f"{who}: field_max >= 1 and field_max * rows * cols <= 2^31 - 1")
        if self.rows > _lib.GG_MATCH_MAX_SIDE or self.cols > _lib.GG_MATCH_MAX_SIDE:
            raise ValueError(f"{who}: the map has more than {_lib.GG_MATCH_MAX_SIDE} rows or columns")

        host_rotations = None
        if rotations is not None:
            host_rotations = _int32_array(who, "rotations", rotations, "[K, 2]", lambda sh: len(sh) == 2 and sh[1] == 2)
            if not 1 <= host_rotations.shape[0] <= _lib.GG_MATCH_MAX_ROTATIONS:
                raise ValueError(f"{who}: rotations holds 1 to {_lib.GG_MATCH_MAX_ROTATIONS} candidates")
            if (np.abs(host_rotations.astype(np.int64)) > _lib.GG_MATCH_UNIT).any():
                raise ValueError(f"{who}: a word of rotations lies outside [-{_lib.GG_MATCH_UNIT}, {_lib.GG_MATCH_UNIT}]")
        K = host_rotations.shape[0] if host_rotations is not None else 1
        if not _is_planes(scan, plane):
            raise ValueError(f"{who}: scan must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(scan.shape[0])
        if not (_is_planes(field, plane) and field.shape[0] == B and field.device == scan.device):
            raise ValueError(f"{who}: field must be a contiguous CUDA torch.int32 tensor of the shape and device of scan")
        host_shifts = _int32_array(who, "shifts", shifts, "[B, 2]", lambda sh: sh == (B, 2)) if shifts is not None else None
        host_pivots = _int32_array(who, "pivots", pivots, "[B, 2]", lambda sh: sh == (B, 2)) if pivots is not None else None
        if host_pivots is not None and ((host_pivots < 0) | (host_pivots >= np.array([self.rows, self.cols]))).any():
            raise ValueError(f"{who}: a pivot lies outside the map")
        D = 2 * int(window) + 1
        want = {"best": (B, 6), "scores": (B, K, D, D) if scores else None}
        res = _reuse_outputs(who, out if out is not None else MatchOutputs(), want, scan.device, [scan.data_ptr(), field.data_ptr()])
        self._torch_used = True
        x = _lib.GGPlaneMatches()
        cells = self.rows * self.cols
        x.n, x.d_scan, x.scan_stride, x.d_field, x.field_stride = B, scan.data_ptr(), cells, field.data_ptr(), cells
        x.field_max, x.window = int(field_max), int(window)
        if host_shifts is not None:
            x.shifts = _int32_ptr(host_shifts)
        if host_pivots is not None:
            x.pivots = _int32_ptr(host_pivots)
        if host_rotations is not None:
            x.rotations, x.n_rotations = _int32_ptr(host_rotations), K
        x.order = c_order
        x.d_best = res.best.data_ptr()
        x.d_scores, x.score_stride = (res.scores.data_ptr(), K * D * D) if scores else (None, 0)
        stream = self._stream_arg(on_torch_stream, scan.device)
        _check(self._L, self._ctx, self._L.gg_match_planes(self._ctx, C.byref(x), stream), "gg_match_planes")
        return res

    def footprint_planes(self, blocked, spans, *, min_fit: Optional[int] = None, outside_free: bool = False, order: str = "row", mask: bool = True,
                         fit: bool = True, counts: bool = True, out: Optional[FootprintOutputs] = None, on_torch_stream: bool = False) -> FootprintOutputs:
        """Which headings of a vehicle footprint fit at every cell of many maps (gg_footprint_planes).  blocked: a contiguous CUDA
        torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"), B <= n_slots: a cell is blocked where the word is >= 0 --
        FusionOutputs.state, VisibilityOutputs.state or ClusterOutputs.cell_cluster as it is, the convention of route_planes.  spans:
        footprint_spans(...), int32 [K, 2 R + 1, 2] with 1 <= K <= 32 and 0 <= R <= 32, shared by all maps: row a + R of heading k is
        (lo, hi), the cells (a, lo .. hi) of the footprint in (row, col) offsets from the reference cell, lo > hi an empty row; every
        heading must be column-convex.  Heading k fits at (r, c) iff no cell (r + a, c + b) of its footprint is blocked; a cell outside
        the map is blocked, or free with outside_free=True.
        mask int32 [B, rows, cols]: bit k set iff heading k fits (the uint32 word of the C call, same bits).  fit int32: -1 where at
        least min_fit headings fit, else their number -- a `blocked` plane of route_planes and a seed plane of clearance_planes as it is;
        min_fit=None means K ("fits at every heading", the conservative plane), min_fit=1 "fits at some heading", the exact projection
        of the configuration space.  counts int32 [B, 3]: cells where all K fit, where at least min_fit fit, where none fits.  At least
        one of the three must be asked for.  `out`: a FootprintOutputs of an earlier call with the same arguments, whose tensors are
        reused; it may not hold the input.  Bit operations and integer sums only: bit-identical from run to run.  Enqueued on the
        context's own stream or, with on_torch_stream=True, on the current torch stream; nothing synchronises.  No map is read or
        changed."""
        who = "footprint_planes"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        if not isinstance(outside_free, (bool, np.bool_)):
            raise ValueError(f"{who}: outside_free is True or False")
        host_spans = _int32_array(who, "spans", spans, "[K, 2 R + 1, 2]", lambda sh: len(sh) == 3 and sh[2] == 2 and sh[1] % 2 == 1)
        K, R = int(host_spans.shape[0]), int(host_spans.shape[1]) // 2
        if not 1 <= K <= _lib.GG_FOOTPRINT_MAX_HEADINGS or R > _lib.GG_FOOTPRINT_MAX_RADIUS:
            raise ValueError(f"{who}: spans hold 1 to {_lib.GG_FOOTPRINT_MAX_HEADINGS} headings of radius 0 to {_lib.GG_FOOTPRINT_MAX_RADIUS}")
        if min_fit is None:
            min_fit = K
        if isinstance(min_fit, bool) or not isinstance(min_fit, (int, np.integer)) or not 1 <= min_fit <= K:
            raise ValueError(f"{who}: min_fit is an integer in [1, {K}] or None")
        if not (mask or fit or counts):
            raise ValueError(f"{who}: at least one of mask, fit and counts must be asked for")
        if not _is_planes(blocked, plane):
            raise ValueError(f"{who}: blocked must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(blocked.shape[0])
        want = {"mask": (B,) + plane if mask else None, "fit": (B,) + plane if fit else None, "counts": (B, 3) if counts else None}
        res = _reuse_outputs(who, out if out is not None else FootprintOutputs(), want, blocked.device, [blocked.data_ptr()], in_place="is the input of the call")
        self._torch_used = True
        x = _lib.GGPlaneFootprints()
        cells = self.rows * self.cols
        x.n, x.d_blocked, x.blocked_stride = B, blocked.data_ptr(), cells
        x.spans, x.n_headings, x.radius = _int32_ptr(host_spans), K, R
        x.min_fit, x.outside_free = int(min_fit), int(bool(outside_free))
        x.order = c_order
        x.d_mask, x.mask_stride = (res.mask.data_ptr(), cells) if mask else (None, 0)
        x.d_fit, x.fit_stride = (res.fit.data_ptr(), cells) if fit else (None, 0)
        x.d_counts = res.counts.data_ptr() if counts else None
        stream = self._stream_arg(on_torch_stream, blocked.device)
        _check(self._L, self._ctx, self._L.gg_footprint_planes(self._ctx, C.byref(x), stream), "gg_footprint_planes")
        return res

    def route_headings(self, mask, goals, moves, cost=None, *, goal_headings: int = 0xFFFFFFFF, cost_max: int = 252, max_cost: int = 0,
                       order: str = "row", next: bool = True, best: bool = True, counts: bool = True, starts=None, max_len: int = 0,
                       out: Optional[HeadingOutputs] = None, on_torch_stream: bool = False) -> HeadingOutputs:
        """The navigation function of a state lattice over cells and headings of many maps (gg_route_headings): per cell and heading the
        exact cost of the cheapest chain of moves to a goal state, every state on it one the heading mask admits.  mask: a contiguous CUDA
        torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"), B <= n_slots: state (k, cell) is admissible where bit k is
        set -- FootprintOutputs.mask as it is.  goals: same shape: a goal cell where the word is >= 0 -- FusionOutputs.frontier as it is, or
        goal_planes(); heading k of a goal cell is a goal state where bit k of goal_headings is set and the state is admissible.  moves:
        heading_moves(...), int32 [K, 8, 4] with 1 <= K <= 32, shared by all maps: entry m of heading k = (da, db, k2, s) leads from
        (k, (r, c)) to (k2, (r + da, c + db)) at s * min(max(cost word, 1), cost_max) of the cell entered (cost None: 1 everywhere);
        s == 0 marks an absent entry.  The cells between the ends of a move longer than one cell are not looked at: pad the footprint.
        dist [B, K, rows, cols] is _lib.GG_ROUTE_NONE on an inadmissible state, where no chain leads to a goal, or where it costs more
        than max_cost > 0.  next: the smallest slot whose move attains dist, _lib.GG_HEADINGS_AT_GOAL on a goal state, -1 unreached.
        best / best_heading [B, rows, cols]: the least dist over the headings and the smallest heading that attains it (-1: none).
        counts int32 [B, 3]: goal, reached and admissible states.
        starts: [B, 2] (linear cell index in `order` or -1, heading): with max_len >= 1, paths [B, max_len, 2] holds the (cell, heading)
        pairs from the start state to the goal state and path_len [B] the length of the whole path (0: unreached); the pairs from path_len
        on keep what they held (-1 in a tensor this call allocates).
        The limit max s * cost_max * rows * cols * K <= 2^31 - 2 keeps every sum inside an int32.  next=False / best=False / counts=False
        leave those out (None).  `out`: a HeadingOutputs of an earlier call with the same arguments, whose tensors are reused; it may not
        hold an input.  Integer arithmetic only: bit-identical from run to run.  Enqueued on the context's own stream or, with
        on_torch_stream=True, on the current torch stream; nothing synchronises.  No map is read or changed."""
        who = "route_headings"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, goal_headings=goal_headings, cost_max=cost_max, max_cost=max_cost, max_len=max_len)
        if not 0 <= goal_headings <= 0xFFFFFFFF:
            raise ValueError(f"{who}: goal_headings is a uint32 mask")
        if not 1 <= cost_max <= _lib.GG_ROUTE_NONE:
            raise ValueError(f"{who}: cost_max >= 1")
        if not 0 <= max_cost <= _lib.GG_ROUTE_NONE:
            raise ValueError(f"{who}: max_cost lies in [0, 2^31 - 1]")
        if max_len < 0 or max_len > _lib.GG_ROUTE_NONE or (starts is None and max_len != 0):
            raise ValueError(f"{who}: max_len is >= 1 with starts and 0 without")
        host_moves = _int32_array(who, "moves", moves, "[K, 8, 4]",
                                  lambda sh: len(sh) == 3 and sh[1:] == (_lib.GG_HEADINGS_MAX_MOVES, 4) and 1 <= sh[0] <= _lib.GG_HEADINGS_MAX,
                                  suffix=f" with 1 <= K <= {_lib.GG_HEADINGS_MAX}")
        K = int(host_moves.shape[0])
        present = host_moves[:, :, 3] != 0
        s = host_moves[:, :, 3][present]
        if ((s < 1) | (s > _lib.GG_HEADINGS_MAX_COST)).any():
            raise ValueError(f"{who}: a move's cost lies outside [1, {_lib.GG_HEADINGS_MAX_COST}]")
        if (np.abs(host_moves[:, :, :2][present]) > _lib.GG_HEADINGS_MAX_STEP).any():
            raise ValueError(f"{who}: a move is longer than {_lib.GG_HEADINGS_MAX_STEP} cells")
        k2 = host_moves[:, :, 2]
        if ((k2 < 0) | (k2 >= K))[present].any():
            raise ValueError(f"{who}: a move's heading lies outside [0, K)")
        own = (host_moves[:, :, 0] == 0) & (host_moves[:, :, 1] == 0) & (k2 == np.arange(K)[:, None])
        if (own & present).any():
            raise ValueError(f"{who}: a move leads to its own state")
        if (int(s.max()) if s.size else 0) * cost_max * self.rows * self.cols * K > _lib.GG_HEADINGS_LIMIT:
            raise ValueError(f"{who}: max s * cost_max * rows * cols * K exceeds 2^31 - 2")
        if not _is_planes(mask, plane):
            raise ValueError(f"{who}: mask must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(mask.shape[0])
        for name, t in (("goals", goals), ("cost", cost)):
            if (t is not None or name == "goals") and not (_is_planes(t, plane) and t.shape[0] == B and t.device == mask.device):
                raise ValueError(f"{who}: {name} must be a contiguous CUDA torch.int32 tensor of the shape and device of mask")
        host_starts = None
        if starts is not None:
            host_starts = _int32_array(who, "starts", starts, "[B, 2]", lambda sh: sh == (B, 2))
            cell, heading = host_starts[:, 0], host_starts[:, 1]
            if ((cell < -1) | (cell >= self.rows * self.cols)).any():
                raise ValueError(f"{who}: a start cell lies outside [-1, rows * cols)")
            if ((cell >= 0) & ((heading < 0) | (heading >= K))).any():
                raise ValueError(f"{who}: a start heading lies outside [0, K)")
            if max_len < 1:
                raise ValueError(f"{who}: starts needs max_len >= 1")
        with_paths = host_starts is not None
        want = {"dist": (B, K) + plane, "next": (B, K) + plane if next else None, "best": (B,) + plane if best else None,
                "best_heading": (B,) + plane if best else None, "counts": (B, 3) if counts else None,
                "paths": (B, max_len, 2) if with_paths else None, "path_len": (B,) if with_paths else None}
        # (the call leaves the pairs behind a path alone: -1 in a tensor allocated here)
        res = _reuse_outputs(who, out if out is not None else HeadingOutputs(), want, mask.device, [t.data_ptr() for t in (mask, goals, cost) if t is not None],
                             fill={"paths": -1})
        self._torch_used = True
        x = _lib.GGHeadingRoutes()
        cells = self.rows * self.cols
        x.n, x.d_mask, x.mask_stride, x.d_goals, x.goal_stride = B, mask.data_ptr(), cells, goals.data_ptr(), cells
        x.d_cost, x.cost_stride = (cost.data_ptr(), cells) if cost is not None else (None, 0)
        x.goal_headings, x.n_headings, x.moves = int(goal_headings), K, _int32_ptr(host_moves)
        x.cost_max, x.max_cost = int(cost_max), int(max_cost)
        x.order = c_order
        x.d_dist, x.dist_stride, x.plane_stride = res.dist.data_ptr(), K * cells, cells
        if next:
            x.d_next, x.next_stride, x.next_plane_stride = res.next.data_ptr(), K * cells, cells
        if best:
            x.d_best, x.best_stride, x.d_best_heading, x.best_heading_stride = res.best.data_ptr(), cells, res.best_heading.data_ptr(), cells
        x.d_counts = res.counts.data_ptr() if counts else None
        if with_paths:
            x.starts = _int32_ptr(host_starts)
            x.d_paths, x.path_stride, x.max_len, x.d_path_len = res.paths.data_ptr(), 2 * int(max_len), int(max_len), res.path_len.data_ptr()
        stream = self._stream_arg(on_torch_stream, mask.device)
        _check(self._L, self._ctx, self._L.gg_route_headings(self._ctx, C.byref(x), stream), "gg_route_headings")
        return res

    def score_rollouts(self, mask, table, starts, *, rotations=None, relative: bool = True, cost=None, dist=None, clear=None,
                       cost_max: int = 252, reach: int = 0, order: str = "row", step_major: bool = False, best: bool = True,
                       out: Optional[RolloutOutputs] = None, on_torch_stream: bool = False, stream=None) -> RolloutOutputs:
        """The score of candidate trajectories of many maps (gg_score_rollouts): which rollouts of a table fit the heading mask pose by
        pose, what they cost on the cost plane, their least clearance, the cost-to-go of route_headings at their end, and the best of
        every map.  mask: a contiguous CUDA torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"), B <= n_slots --
        FootprintOutputs.mask as it is.  table: a CUDA torch.int32 tensor [P, T, 4] (one library for all maps) or [B, P, T, 4] (per-map
        samples), entry (p, t) = (da, db, dk, s), 1 <= P <= 65536, 1 <= T <= 128; the call reads it step-major, so it is permuted with
        one device copy on the current torch stream (and, unless the call is enqueued on that stream, the method waits for the copy)
        unless step_major=True says it already is [T, P, 4] / [B, T, P, 4] and contiguous.  A rollout ends before its first entry with
        s <= 0.  starts: [B, 3] host integers (r16, c16, k0): the position in 1/16 cell (16 * row + 8: a cell centre) and the heading;
        r16 == -1: no start.  relative=True: the entries are offsets in the start pose's frame, rotated by heading k0 of `rotations`
        (rotation_table(angles), int32 [K, 2]; required) and dk is added to k0 modulo K -- rollout_arcs() makes such a library.
        relative=False: the entries are absolute (r16, c16, heading); K is then taken from `rotations` when given, else from dist.
        cost: planes like mask, w = min(max(word, 1), cost_max), None: 1; a step costs min(s, 32767) * w of its cell.  dist:
        HeadingOutputs.dist [B, K, rows, cols] as it is, None: togo = 0.  clear: ClearanceOutputs.dist2 as it is, or None.  reach R > 0:
        poses more than R rows or columns from the start's cell are inadmissible (R <= 63).  The cells between consecutive poses are not
        looked at: pad the footprint.  records int32 [B, P, 8]: steps (leading admissible poses), len, cost, end_cell (linear index in
        `order`), end_heading, togo (dist at the end of a complete rollout, _lib.GG_ROUTE_NONE otherwise), clear, total = cost + togo
        (_lib.GG_ROUTE_NONE unless complete and reached); RolloutOutputs.table(b) names them.  best int32 [B, 4]: the smallest p of
        least total (-1: none), that total, the complete and the scored rollouts; best=False leaves it out (None).  The limit
        T * 32767 * cost_max <= 2^31 - 2 keeps every cost inside an int32.  `out`: a RolloutOutputs of an earlier call with the same
        arguments, whose tensors are reused; it may not hold an input.  Integer arithmetic only: bit-identical from run to run.
        Enqueued on the context's own stream, with on_torch_stream=True on the current torch stream, or on `stream` (a raw handle);
        nothing else synchronises.  No map is read or changed."""
        import torch

        who = "score_rollouts"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, cost_max=cost_max, reach=reach)
        if not 0 <= reach <= _lib.GG_ROLLOUTS_MAX_REACH:
            raise ValueError(f"{who}: reach lies in [0, {_lib.GG_ROLLOUTS_MAX_REACH}]")
        if not 1 <= cost_max <= _lib.GG_ROUTE_NONE:
            raise ValueError(f"{who}: cost_max >= 1")
        if not _is_planes(mask, plane):
            raise ValueError(f"{who}: mask must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B = int(mask.shape[0])
        for name, t in (("cost", cost), ("clear", clear)):
            if t is not None and not (_is_planes(t, plane) and t.shape[0] == B and t.device == mask.device):
                raise ValueError(f"{who}: {name} must be a contiguous CUDA torch.int32 tensor of the shape and device of mask")
        host_rot = None
        if rotations is not None:
            host_rot = _int32_array(who, "rotations", rotations, "[K, 2]", lambda sh: len(sh) == 2 and sh[1] == 2 and 1 <= sh[0] <= _lib.GG_HEADINGS_MAX,
                                    f" with 1 <= K <= {_lib.GG_HEADINGS_MAX}")
            if int(np.abs(host_rot).max()) > _lib.GG_MATCH_UNIT:
                raise ValueError(f"{who}: a rotation word lies outside [-{_lib.GG_MATCH_UNIT}, {_lib.GG_MATCH_UNIT}]")
        elif relative:
            raise ValueError(f"{who}: the relative frame needs rotations")
        if dist is not None and not (torch.is_tensor(dist) and dist.dim() == 4 and 1 <= dist.shape[1] <= _lib.GG_HEADINGS_MAX
                                     and _is_dense(dist, (B, int(dist.shape[1])) + plane, device=mask.device)):
            raise ValueError(f"{who}: dist must be a contiguous CUDA torch.int32 tensor [B, K, {plane[0]}, {plane[1]}] on the device of mask")
        if host_rot is None and dist is None:
            raise ValueError(f"{who}: the number of headings comes from rotations or from dist: give one of them")
        K = int(host_rot.shape[0]) if host_rot is not None else int(dist.shape[1])
        if dist is not None and int(dist.shape[1]) != K:
            raise ValueError(f"{who}: dist has {int(dist.shape[1])} headings and rotations {K}")
        if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int32 and table.dim() in (3, 4) and table.shape[-1] == 4
                and table.device == mask.device and (table.dim() == 3 or table.shape[0] == B)):
            raise ValueError(f"{who}: table must be a CUDA torch.int32 tensor [P, T, 4] or [B, P, T, 4] on the device of mask")
        P, T = (int(table.shape[-2]), int(table.shape[-3])) if step_major else (int(table.shape[-3]), int(table.shape[-2]))
        if not 1 <= P <= _lib.GG_ROLLOUTS_MAX or not 1 <= T <= _lib.GG_ROLLOUTS_MAX_STEPS:
            raise ValueError(f"{who}: a table of {P} rollouts of {T} steps: 1 <= P <= {_lib.GG_ROLLOUTS_MAX} and 1 <= T <= {_lib.GG_ROLLOUTS_MAX_STEPS}")
        if step_major and not table.is_contiguous():
            raise ValueError(f"{who}: a step-major table must be contiguous")
        if T * 32767 * cost_max > _lib.GG_ROLLOUTS_LIMIT:
            raise ValueError(f"{who}: T * 32767 * cost_max exceeds 2^31 - 2")
        host_starts = _int32_array(who, "starts", starts, "[B, 3]", lambda sh: sh == (B, 3))
        given = host_starts[:, 0] != -1
        r16, c16, k0 = (host_starts[given, j] for j in range(3))
        if ((r16 < 0) | (r16 >= 16 * self.rows) | (c16 < 0) | (c16 >= 16 * self.cols)).any():
            raise ValueError(f"{who}: a start lies outside the map")
        if ((k0 < 0) | (k0 >= K)).any():
            raise ValueError(f"{who}: a start heading lies outside [0, K)")
        want = {"records": (B, P, _lib.GG_ROLLOUTS_RECORD_WORDS), "best": (B, 4) if best else None}
        res = _reuse_outputs(who, out if out is not None else RolloutOutputs(), want, mask.device,
                             [t.data_ptr() for t in (mask, cost, dist, clear, table) if t is not None])
        self._torch_used = True
        own_torch_stream = on_torch_stream and stream is None
        if step_major:
            res.step_major = table
        else:
            with torch.cuda.device(mask.device):
                res.step_major = table.transpose(-3, -2).contiguous()
                if not own_torch_stream:
                    torch.cuda.current_stream(mask.device).synchronize()
        x = _lib.GGRollouts()
        cells = self.rows * self.cols
        x.n, x.d_mask, x.mask_stride = B, mask.data_ptr(), cells
        x.d_cost, x.cost_stride = (cost.data_ptr(), cells) if cost is not None else (None, 0)
        x.d_dist, x.dist_stride, x.plane_stride = (dist.data_ptr(), K * cells, cells) if dist is not None else (None, 0, 0)
        x.d_clear, x.clear_stride = (clear.data_ptr(), cells) if clear is not None else (None, 0)
        x.n_headings, x.starts = K, _int32_ptr(host_starts)
        x.rotations = _int32_ptr(host_rot) if host_rot is not None else None
        x.frame = _lib.GG_ROLLOUTS_RELATIVE if relative else _lib.GG_ROLLOUTS_ABSOLUTE
        x.d_table, x.table_stride = res.step_major.data_ptr(), 4 * P * T if table.dim() == 4 else 0
        x.n_rollouts, x.n_steps, x.cost_max, x.reach, x.order = P, T, int(cost_max), int(reach), c_order
        x.d_records, x.record_stride = res.records.data_ptr(), _lib.GG_ROLLOUTS_RECORD_WORDS * P
        x.d_best = res.best.data_ptr() if best else None
        handle = self._stream_arg(on_torch_stream or stream is not None, mask.device, handle=stream)
        _check(self._L, self._ctx, self._L.gg_score_rollouts(self._ctx, C.byref(x), handle), "gg_score_rollouts")
        return res

    def track_clusters(self, cell_cluster, previous: Optional[TrackOutputs] = None, shifts=None, max_clusters: int = 256, gate: int = 1,
                       cell_track: bool = False, out: Optional[TrackOutputs] = None, on_torch_stream: bool = False, *,
                       order: str = "row") -> TrackOutputs:
        """Which object is which (gg_track_clusters): this scan's clusters associated with the last scan's.  cell_cluster: a contiguous
        CUDA torch.int32 tensor [B, rows, cols] ([B, cols, rows] with order="col"), B <= n_slots -- ClusterOutputs.cell_cluster as it is:
        -1 or the cell's cluster id; ids from max_clusters on belong to no cluster.  previous: the TrackOutputs of the last frame's call
        (same B, max_clusters and order), or None for no prior: every cluster is then born, with ids 0, 1, ... in cluster order.  shifts:
        what move_maps returned for the move between the two scans, [B, 2], or None for no move, with the meaning it has in fuse_states.
        A current cluster c and a previous cluster p overlap by the number of (cell of c, offset within `gate` cells) pairs that land
        on a cell of p; c names the p it overlaps most (the smallest among equals), p keeps the claimant that overlaps it most (the
        smallest among equals), and that claimant inherits p's track id with age + 1; every other cluster gets a fresh id.
        tracks int32 [B, max_clusters, 8]: per cluster track_id, age, prev, overlap, still (the gate-0 part of overlap), cells, sum_row,
        sum_col -- TrackOutputs.table(b) gives them as records; heads int32 [B, 4]: the next fresh id, the clusters, born, ended;
        cell_track=True adds the plane of track ids (-1 on a cell of no cluster).  The result keeps a reference to cell_cluster: the next
        call reads it as its previous scan, so the caller alternates between two id planes (cluster_clouds(out=...)) and two
        TrackOutputs.  `out`: a TrackOutputs of an earlier call with the same arguments, whose tensors are reused; it may not be
        `previous`.  Integer arithmetic only: bit-identical from run to run.  Enqueued on the context's own stream or, with
        on_torch_stream=True, on the current torch stream; nothing synchronises.  No map is read or changed."""
        who = "track_clusters"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        _check_integers(who, max_clusters=max_clusters, gate=gate)
        if not 1 <= max_clusters <= _lib.GG_TRACK_MAX_CLUSTERS:
            raise ValueError(f"{who}: max_clusters lies in [1, {_lib.GG_TRACK_MAX_CLUSTERS}]")
        if not 0 <= gate <= _lib.GG_TRACK_MAX_GATE:
            raise ValueError(f"{who}: gate lies in [0, {_lib.GG_TRACK_MAX_GATE}]")
        if not _is_planes(cell_cluster, plane):
            raise ValueError(f"{who}: cell_cluster must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B, M = int(cell_cluster.shape[0]), int(max_clusters)
        if previous is not None:
            if out is previous:
                raise ValueError(f"{who}: out is `previous`: no update in place is defined, alternate between two TrackOutputs")
            if previous.order != order:
                raise ValueError(f"{who}: previous was computed with order={previous.order!r}")
            if not all(_is_dense(t, sh, device=cell_cluster.device) for t, sh in ((previous.cell_cluster, (B,) + plane), (previous.tracks, (B, M, 8)), (previous.heads, (B, 4)))):
                raise ValueError(f"{who}: previous must be the TrackOutputs of a call with the same B, max_clusters and order")
        host_shifts = _int32_array(who, "shifts", shifts, "[B, 2]", lambda sh: sh == (B, 2)) if shifts is not None else None
        want = {"tracks": (B, M, 8), "heads": (B, 4), "cell_track": (B,) + plane if cell_track else None}
        inputs = [cell_cluster.data_ptr()] + ([previous.cell_cluster.data_ptr(), previous.tracks.data_ptr(), previous.heads.data_ptr()] if previous is not None else [])
        res = _reuse_outputs(who, out if out is not None else TrackOutputs(), want, cell_cluster.device, inputs)
        res.cell_cluster, res.order = cell_cluster, order
        self._torch_used = True
        cells = self.rows * self.cols
        x = _lib.GGClusterTracks()
        x.n, x.d_cells, x.cells_stride = B, cell_cluster.data_ptr(), cells
        if previous is not None:
            x.d_cells_prev, x.prev_stride = previous.cell_cluster.data_ptr(), cells
            x.d_tracks_in, x.d_heads_in = previous.tracks.data_ptr(), previous.heads.data_ptr()
        if host_shifts is not None:
            x.shifts = _int32_ptr(host_shifts)
        x.max_clusters, x.gate = M, int(gate)
        x.order = c_order
        x.d_tracks_out, x.d_heads_out = res.tracks.data_ptr(), res.heads.data_ptr()
        if cell_track:
            x.d_cell_track, x.track_stride = res.cell_track.data_ptr(), cells
        stream = self._stream_arg(on_torch_stream, cell_cluster.device)
        _check(self._L, self._ctx, self._L.gg_track_clusters(self._ctx, C.byref(x), stream), "gg_track_clusters")
        return res

    def cluster_planes(self, seeds, *, lo: int = 0, hi: Optional[int] = None, connectivity: int = 8, min_cells: int = 1, values=None,
                       max_regions: int = 256, order: str = "row", sizes: bool = False, out: Optional[RegionOutputs] = None,
                       on_torch_stream: bool = False) -> RegionOutputs:
        """The connected regions of planes the caller holds (gg_cluster_planes).  seeds: a contiguous CUDA torch.int32 tensor [B, rows,
        cols] ([B, cols, rows] with order="col"), B <= n_slots; a cell is a member where lo <= word <= hi (hi=None: INT32_MAX, so the
        default is the ">= 0" rule of clearance_planes: FusionOutputs.frontier or an id plane as it is; lo=hi=1: the occupied cells of
        a state plane).  The members' connected components under `connectivity` 4 or 8 of at least min_cells cells are the regions,
        numbered by ascending smallest linear cell index of `order`; smaller components are dropped.  cell_cluster: -1 or the region's
        id -- what track_clusters and clearance_planes take as it stands; cell_size (with sizes=True, and always with min_cells > 1,
        whose working memory it is): 0 or the size of the cell's component, dropped ones too; heads int32 [B, 4]: regions, dropped
        components, member cells, kept cells; regions int32 [B, max_regions, 12] (max_regions=0: None): gg_region records --
        RegionOutputs.table(b) gives them as REGION_DTYPE records with the int64 coordinate sums, centroids() in metres.  values: a
        tensor like seeds (RouteOutputs.dist as it is): value_min is its minimum over a region and value_cell the cell that attains
        it, the smallest index among equals -- the goal to hand to goal_planes(); without it INT32_MAX and -1.  `out`: a RegionOutputs
        of an earlier call with the same arguments, whose tensors are reused; neither seeds nor values may be one of them.  Integer
        arithmetic only: bit-identical from run to run.  Enqueued on the context's own stream or, with on_torch_stream=True, on the
        current torch stream; nothing synchronises.  No map is read or changed."""
        who = "cluster_planes"
        plane, c_order = _plane_order(who, order, self.rows, self.cols)
        hi = 0x7FFFFFFF if hi is None else hi
        _check_integers(who, lo=lo, hi=hi, connectivity=connectivity, min_cells=min_cells, max_regions=max_regions)
        if not -(1 << 31) <= lo <= hi <= 0x7FFFFFFF:
            raise ValueError(f"{who}: -2^31 <= lo <= hi <= 2^31 - 1")
        if connectivity not in (4, 8):
            raise ValueError(f"{who}: connectivity is 4 or 8")
        if not 1 <= min_cells <= 0x7FFFFFFF:
            raise ValueError(f"{who}: min_cells is an integer >= 1")
        if not 0 <= max_regions <= 0x7FFFFFFF:
            raise ValueError(f"{who}: max_regions is an integer >= 0")
        if not _is_planes(seeds, plane):
            raise ValueError(f"{who}: seeds must be a contiguous CUDA torch.int32 tensor [B, {plane[0]}, {plane[1]}]")
        B, M = int(seeds.shape[0]), int(max_regions)
        if values is not None and not _is_dense(values, (B,) + plane, device=seeds.device):
            raise ValueError(f"{who}: values must be a contiguous CUDA torch.int32 tensor of the shape of seeds, on their device")
        with_sizes = bool(sizes) or min_cells > 1
        want = {"cell_cluster": (B,) + plane, "cell_size": (B,) + plane if with_sizes else None, "heads": (B, 4),
                "regions": (B, M, 12) if M else None}
        inputs = [seeds.data_ptr()] + ([values.data_ptr()] if values is not None else [])
        res = _reuse_outputs(who, out if out is not None else RegionOutputs(), want, seeds.device, inputs,
                             in_place="is an input of the call: seeds and values may not be outputs")
        self._torch_used = True
        cells = self.rows * self.cols
        x = _lib.GGPlaneClusters()
        x.n, x.d_seeds, x.seed_stride = B, seeds.data_ptr(), cells
        x.lo, x.hi, x.connectivity, x.min_cells, x.order = int(lo), int(hi), int(connectivity), int(min_cells), c_order
        if values is not None:
            x.d_values, x.value_stride = values.data_ptr(), cells
        x.d_cell_cluster, x.plane_stride = res.cell_cluster.data_ptr(), cells
        if with_sizes:
            x.d_cell_size, x.size_stride = res.cell_size.data_ptr(), cells
        x.d_heads = res.heads.data_ptr()
        if M:
            x.d_regions, x.max_regions = res.regions.data_ptr(), M
        stream = self._stream_arg(on_torch_stream, seeds.device)
        _check(self._L, self._ctx, self._L.gg_cluster_planes(self._ctx, C.byref(x), stream), "gg_cluster_planes")
        return res

    def box_clusters(self, points, n_points: Sequence[int], point_cluster, n_clusters, rotations, *, transforms=None, slots=None,
                     first_slot: int = 0, criterion: str = "edge", max_clusters: int = 256, costs: bool = False,
                     out: Optional[BoxOutputs] = None, on_torch_stream: bool = False) -> BoxOutputs:
        """The shape of every object (gg_box_clusters): a rectangle fitted to every cluster of many clouds by a search over candidate
        headings.  points / n_points / transforms / slots / first_slot as for cluster_clouds, which this call follows: point_cluster is
        its ClusterOutputs.point_cluster (contiguous CUDA int32 [B, stride]) and n_clusters its ClusterOutputs.n_clusters (int32 [B]) as
        they stand.  rotations: rotation_table(angles), int32 [K, 2] with 1 <= K <= 32; for a rectangle list angles in [0, pi/2).  A
        point takes part when its id lies in [0, min(n_clusters, max_clusters)) and it lies inside its map; its position is quantised
        to 16 units per cell relative to the map's position and projected on every heading.  criterion "area": the heading of the
        smallest rectangle; "edge": the heading under which the points lie closest to the rectangle's edges (the L-shape of a car seen
        from one corner); among equal costs the earlier table entry.  boxes int32 [B, max_clusters, 8]: heading, points, a_min, a_max,
        b_min, b_max, cost_lo, cost_hi per cluster (heading -1 and zeros for a cluster without a point; BoxOutputs.metric gives centre,
        length, width and yaw in metres); costs=True adds int64 [B, max_clusters, K], the bits of every uint64 cost (-1: no point).
        Records and rows from min(n_clusters, max_clusters) on are never written.  `out`: a BoxOutputs of an earlier call with the same
        arguments, whose tensors are reused.  Integer arithmetic only: bit-identical from run to run.  Enqueued on the context's own
        stream or, with on_torch_stream=True, on the current torch stream; nothing synchronises.  No map is read beyond its position
        or changed; fresh maps stay fresh."""
        import torch

        who = "box_clusters"
        x = _lib.GGClusterBoxes()
        B, stride, keep = self._labelled_clouds(who, x, points, n_points, None, None, transforms, slots, first_slot, labelled=False)
        if criterion not in _lib.BOX_CRITERIA:
            raise ValueError(f"{who}: criterion is one of {list(_lib.BOX_CRITERIA)}")
        _check_integers(who, max_clusters=max_clusters)
        if not 1 <= max_clusters <= _lib.GG_BOX_MAX_CLUSTERS:
            raise ValueError(f"{who}: max_clusters lies in [1, {_lib.GG_BOX_MAX_CLUSTERS}]")
        rot = _int32_array(who, "rotations", rotations, "[K, 2]", lambda sh: len(sh) == 2 and sh[1] == 2 and 1 <= sh[0] <= _lib.GG_BOX_MAX_HEADINGS,
                           f" with 1 <= K <= {_lib.GG_BOX_MAX_HEADINGS}")
        if int(np.abs(rot).max()) > _lib.GG_MATCH_UNIT:
            raise ValueError(f"{who}: a rotation word lies outside [-{_lib.GG_MATCH_UNIT}, {_lib.GG_MATCH_UNIT}]")
        if not _is_dense(point_cluster, (B, stride), device=points.device):
            raise ValueError(f"{who}: point_cluster must be a contiguous CUDA torch.int32 tensor of shape {(B, stride)}")
        if not _is_dense(n_clusters, (B,), device=points.device):
            raise ValueError(f"{who}: n_clusters must be a contiguous CUDA torch.int32 tensor of shape {(B,)}")
        M, K = int(max_clusters), int(rot.shape[0])
        want = {"boxes": (B, M, 8), "costs": ((B, M, K), torch.int64) if costs else None}
        inputs = [points.data_ptr(), point_cluster.data_ptr(), n_clusters.data_ptr()]
        res = _reuse_outputs(who, out if out is not None else BoxOutputs(), want, points.device, inputs)
        self._torch_used = True
        x.d_point_cluster, x.d_n_clusters = point_cluster.data_ptr(), n_clusters.data_ptr()
        x.rotations, x.n_rotations = _int32_ptr(rot), K
        x.criterion, x.max_clusters = _lib.BOX_CRITERIA.index(criterion), M
        x.d_boxes = res.boxes.data_ptr()
        x.d_costs = res.costs.data_ptr() if costs else None
        stream = self._stream_arg(on_torch_stream, points.device)
        _check(self._L, self._ctx, self._L.gg_box_clusters(self._ctx, C.byref(x), stream), "gg_box_clusters")
        return res

    def snapshot_maps(self, slots=None, first_slot: int = 0, n: Optional[int] = None) -> dict:
        """A checkpoint of the named maps: {"planes": export_layers() of all eleven layers [n, 11, cols, rows] (on the device, enqueued on
        the current torch stream), "positions": their map positions, float64 [n, 2]}.  restore_maps puts it back -- into these maps, other
        maps, or the maps of another GroundSegmentation of the same geometry."""
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        planes = self.export_layers(slots=slots, first_slot=first_slot, n=n)
        positions = np.empty((cnt, 2), dtype=np.float64)
        for k in range(cnt):
            slot = int(keep[k]) if keep is not None else first + k
            x, y = C.c_double(), C.c_double()
            _check(self._L, self._ctx, self._L.gg_get_map_position(self._ctx, slot, C.byref(x), C.byref(y)), "gg_get_map_position")
            positions[k] = (x.value, y.value)
        return {"planes": planes, "positions": positions}

    def restore_maps(self, state: dict, slots=None, first_slot: int = 0):
        """Put a snapshot_maps state into map k = slots[k], or first_slot + k: all eleven layers (import_layers, on the current torch
        stream) and the map positions.  What runs on these maps afterwards continues as if it had run where the state was taken."""
        planes, positions = state["planes"], np.asarray(state["positions"], dtype=np.float64)
        if planes.dim() != 4 or tuple(planes.shape[1:]) != (len(LAYERS), self.cols, self.rows):
            raise ValueError(f"restore_maps: planes of shape {tuple(planes.shape)} do not fit maps of {self.rows} x {self.cols} cells")
        cnt = int(planes.shape[0])
        if positions.shape != (cnt, 2) or (slots is not None and len(slots) != cnt):
            raise ValueError("restore_maps: planes, positions and slots differ in length")
        if planes.device.index != self.device:  # (a map that changes its GPU)
            planes = planes.to(f"cuda:{self.device}")
        self.import_layers(planes.contiguous(), slots=slots, first_slot=first_slot, n=cnt)
        for k in range(cnt):
            self._maps[int(slots[k]) if slots is not None else first_slot + k].setPosition(positions[k, 0], positions[k, 1])

    # -- GroundSegmentation::setConfig (src/GroundSegmentation.cpp:468-471)
    def setConfig(self, config: GGConfig):
        _check(self._L, self._ctx, self._L.gg_set_config(self._ctx, C.byref(config)), "gg_set_config")

    def getConfig(self) -> GGConfig:
        c = GGConfig()
        _check(self._L, self._ctx, self._L.gg_get_config(self._ctx, C.byref(c)), "gg_get_config")
        return c

    # -- per-map configuration: every GroundSegmentation object of the reference has its own setConfig; here every map slot may
    def set_slot_configs(self, configs, slots=None, first_slot: int = 0):
        """Give map k (slots[k], or first_slot + k) its own configuration configs[k].  configs=None: those maps follow the context's
        configuration (setConfig) again -- then `slots` (or first_slot and a count given as configs=None, slots=range) names them.
        Blocks like setConfig; on any error no map's configuration changes."""
        if configs is None:
            if slots is None:
                raise ValueError("set_slot_configs(None) needs the slots to clear")
            arr = None
            n = len(slots)
        else:
            configs = list(configs)
            n = len(configs)
            arr = (GGConfig * max(n, 1))(*configs)
        sl = None
        if slots is not None:
            sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
            if sl.shape[0] != n:
                raise ValueError("slots and configs differ in length")
        rc = self._L.gg_set_slot_configs(self._ctx, n, sl.ctypes.data_as(C.POINTER(C.c_int32)) if sl is not None else None, int(first_slot),
                                         arr)
        _check(self._L, self._ctx, rc, "gg_set_slot_configs")

    def slot_config(self, slot: int):
        """(the configuration map `slot` runs with, True if it is its own / False if it follows the context's)"""
        c, own = GGConfig(), C.c_int(0)
        _check(self._L, self._ctx, self._L.gg_get_slot_config(self._ctx, int(slot), C.byref(c), C.byref(own)), "gg_get_slot_config")
        return c, bool(own.value)

    # -- the score of a labelled cloud: per-map evaluator counters on the device (scripts/eval_groundpoint_classifier.py:95-132)
    def _stream_arg(self, on_torch_stream: bool, device=None, handle=None):
        """The `stream` argument of a C call: None, the context's own stream, or with on_torch_stream the caller's `handle` or, without
        one, the current torch stream of `device` (default: the context's).  0 = torch's default stream = GG_STREAM_DEFAULT: NULL would
        mean the context's own stream to the library."""
        if not on_torch_stream:
            return None
        if handle is None:
            import torch

            handle = torch.cuda.current_stream(self.device if device is None else device).cuda_stream
        return C.c_void_p(handle if handle else _lib.GG_STREAM_DEFAULT)

    def _labelled_clouds(self, who, x, points, n_points, labels, masks, transforms, slots, first_slot, labelled: bool = True):
        """What split_clouds, rasterize_clouds and cluster_clouds (`who`) share: checks points and labels / masks and fills the ten leading
        members of the fresh gg_cloud_* structure `x` (labelled=False, box_clusters: the eight in front of the labels, which `x` does not
        have).  Returns (B, stride, keep): `keep` holds the host arrays `x` points to, and the caller keeps it referenced until the C
        call has returned."""
        import torch

        assert points.is_cuda and points.dtype == torch.uint8 and points.dim() == 3 and points.is_contiguous()
        B, stride, rec = points.shape
        assert rec in (16, 32)
        if labelled:
            if (labels is None) == (masks is None):
                raise ValueError(f"{who}: exactly one of labels and masks")
            given = labels if labels is not None else masks
            want_shape = (B, stride) if labels is not None else (B, (stride + 3) // 4)
            if not (torch.is_tensor(given) and given.is_cuda and given.dtype == torch.uint8 and given.is_contiguous() and tuple(given.shape) == want_shape):
                raise ValueError(f"{who}: {'labels' if labels is not None else 'masks'} must be a contiguous CUDA uint8 tensor of shape {want_shape}")
        keep = [(C.c_int32 * max(B, 1))(*[int(v) for v in n_points])]
        x.n, x.first_slot, x.point_format = B, int(first_slot), _lib.GG_POINT16 if rec == 16 else _lib.GG_POINT32
        x.d_points, x.cloud_stride, x.n_points = points.data_ptr(), stride, keep[0]
        if slots is not None:
            keep.append((C.c_int32 * max(B, 1))(*[int(v) for v in slots]))
            x.slots = keep[-1]
        if transforms is not None:  # [B, 3, 4] map <- cloud frame, as for filter_batch
            keep.append(np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(B, 12)))
            x.transforms = keep[-1].ctypes.data_as(C.POINTER(C.c_double))
        if not labelled:
            return B, stride, keep
        x.d_labels = labels.data_ptr() if labels is not None else None
        x.d_label_masks = masks.data_ptr() if masks is not None else None
        return B, stride, keep

    def _slot_args(self, slots, first_slot, n):
        if slots is not None:
            sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
            return sl.shape[0], sl.ctypes.data_as(C.POINTER(C.c_int32)), sl, 0
        count = self.n_slots - first_slot if n is None else int(n)
        return count, None, None, int(first_slot)

    def set_score_labels(self, ids=None):
        """The label ids that get a bin of their own (default: the keys of evaluate.LABELS, the reference's yaml); every other id is
        counted in one more bin.  Zeroes all counters."""
        from .evaluate import LABELS

        ids = list(LABELS.keys()) if ids is None else [int(i) for i in ids]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        _check(self._L, self._ctx, self._L.gg_set_score_labels(self._ctx, len(ids), arr), "gg_set_score_labels")
        self._score_ids = ids

    def set_scoring(self, slots=None, first_slot: int = 0, n: Optional[int] = None, enable: bool = True):
        """Scoring on / off for the named maps (default: all): every later filter call on such a map adds its returned cloud to the
        map's counters, on the device."""
        if getattr(self, "_score_ids", None) is None and enable:
            self.set_score_labels()
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        _check(self._L, self._ctx, self._L.gg_set_slot_scoring(self._ctx, cnt, ptr, first, 1 if enable else 0), "gg_set_slot_scoring")

    def scores_raw(self, slots=None, first_slot: int = 0, n: Optional[int] = None):
        """(clouds [n], counts [n, 65, 2] uint64) of the named maps: the counters as the library keeps them."""
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        out = (_lib.GGSlotScores * max(cnt, 1))()
        _check(self._L, self._ctx, self._L.gg_get_slot_scores(self._ctx, cnt, ptr, first, out), "gg_get_slot_scores")
        words = np.frombuffer(out, dtype=np.uint64).reshape(max(cnt, 1), 1 + 2 * (_lib.GG_SCORE_MAX_LABELS + 1))[:cnt]
        return words[:, 0].copy(), words[:, 1:].reshape(cnt, _lib.GG_SCORE_MAX_LABELS + 1, 2).copy()

    def scores(self, slots=None, first_slot: int = 0, n: Optional[int] = None, allow_unknown: bool = False):
        """One evaluate.GroundEvaluator per named map, from its device counters.  A returned point whose label id is not in the list
        raises KeyError, like the reference's evaluator, unless allow_unknown."""
        from .evaluate import GroundEvaluator

        clouds, counts = self.scores_raw(slots, first_slot, n)
        ids = self._score_ids
        return [GroundEvaluator.from_device_counts(ids, counts[k, : len(ids) + 1], int(clouds[k]), allow_unknown) for k in range(len(clouds))]

    def reset_scores(self, slots=None, first_slot: int = 0, n: Optional[int] = None):
        """Zero the counters of the named maps (default: all); scoring stays on or off as it was."""
        cnt, ptr, keep, first = self._slot_args(slots, first_slot, n)
        _check(self._L, self._ctx, self._L.gg_reset_slot_scores(self._ctx, cnt, ptr, first), "gg_reset_slot_scores")

    def score_kernel_time(self, reset: bool = True):
        """(ms, launches) of k_score accumulated under set_flags(profile=True), next to kernel_times()."""
        ms, ln = C.c_double(0.0), C.c_int64(0)
        _check(self._L, self._ctx, self._L.gg_get_score_kernel_time(self._ctx, C.byref(ms), C.byref(ln), 1 if reset else 0), "gg_get_score_kernel_time")
        return ms.value, ln.value

    def set_flags(self, minimal_layers: bool = False, profile: bool = False, concurrent_halves: bool = False, eager_layers: bool = False):
        """gg_set_flags.  minimal_layers: maxGroundHeight / groundCandidates / planeDist -- written by insert_cloud
        (src/GroundSegmentation.cpp:296,303,307) and read by nothing on the path -- are computed when a layer getter asks for one of
        them instead of for every cloud; every getter still returns what the reference's layer would hold.  profile: per-kernel
        events (kernel_times).  filter_batch (device-resident clouds) does that by default; eager_layers switches it back to all nine
        per-call layers per cloud."""
        f = ((_lib.GG_FLAG_MINIMAL_LAYERS if minimal_layers else 0) | (_lib.GG_FLAG_PROFILE if profile else 0) |
             (_lib.GG_FLAG_CONCURRENT_HALVES if concurrent_halves else 0) | (_lib.GG_FLAG_EAGER_LAYERS if eager_layers else 0))
        _check(self._L, self._ctx, self._L.gg_set_flags(self._ctx, f), "gg_set_flags")

    def expected_points(self) -> np.ndarray:
        buf = np.empty(self.rows * self.cols, dtype=np.float32)
        _check(self._L, self._ctx, self._L.gg_get_expected_points(self._ctx, buf.ctypes.data), "gg_get_expected_points")
        return buf.reshape((self.rows, self.cols), order="F")

    # -- GroundSegmentation::filter_cloud (include/groundgrid/GroundSegmentation.h:54)
    def _host_buffers(self, n: int, reuse: bool):
        """Output arrays of one host-buffer call: fresh ones, or (reuse=True) this object's own, grown on demand -- a caller that
        looks at one result before asking for the next (a sensor loop) then pays no allocation and no first-touch page faults
        per cloud (3.8 MB per HDL-64E revolution); the returned arrays are views that the next reuse=True call overwrites."""
        m = max(n, 1)
        if not reuse:
            return np.empty(m * 32, dtype=np.uint8).view(POINT_DTYPE), np.empty(m, dtype=np.uint8), np.empty(m, dtype=np.int32)
        if getattr(self, "_hb_cap", 0) < m:
            self._hb_cap = m + m // 8
            self._hb = (np.zeros(self._hb_cap * 32, dtype=np.uint8).view(POINT_DTYPE), np.zeros(self._hb_cap, dtype=np.uint8),
                        np.zeros(self._hb_cap, dtype=np.int32))
        return self._hb

    def filter_cloud(self, cloud: np.ndarray, cloudOrigin: Sequence[float], mapToBase_z: float, map: Optional[GridMap] = None,
                     return_details: bool = False, map_from_cloud=None, reuse_buffers: bool = False):
        """cloud: POINT_DTYPE array in the map frame.  Returns the segmented cloud (intensity = 49 ground /
        99 non-ground; order kept, ignored, outliers).  With return_details also (labels, out_index)."""
        assert cloud.dtype == POINT_DTYPE, "cloud must use groundgrid_amd.synth.POINT_DTYPE (PointXYZIR, 32 B)"
        gm = map if map is not None else self._maps[0]
        cloud = np.ascontiguousarray(cloud)
        n = cloud.shape[0]
        out, labels, index = self._host_buffers(n, reuse_buffers)
        out_n = C.c_size_t(0)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        # (the per-point labels / positions are copied out only when asked for: the reference's call returns the cloud alone)
        lab_p, idx_p = (labels.ctypes.data, index.ctypes.data) if return_details else (None, None)
        if map_from_cloud is None:
            rc = self._L.gg_filter_cloud(self._ctx, gm.slot, cloud.ctypes.data, n, org, float(mapToBase_z),
                                         out.ctypes.data, C.byref(out_n), lab_p, idx_p)
        else:  # cloud still in the sensor frame: 3x4 (R | t) of map <- cloud frame, transformed on the device
            tf = (C.c_double * 12)(*[float(v) for v in np.asarray(map_from_cloud, dtype=np.float64).reshape(-1)[:12]])
            rc = self._L.gg_filter_cloud_tf(self._ctx, gm.slot, cloud.ctypes.data, n, tf, org, float(mapToBase_z),
                                            out.ctypes.data, C.byref(out_n), lab_p, idx_p)
        _check(self._L, self._ctx, rc, "gg_filter_cloud")
        seg = out[: out_n.value]
        if return_details:
            return seg, labels[:n], index[:n]
        return seg

    segment = filter_cloud  # BASELINE.json's north_star calls the entry point segment(); same thing

    def alloc_layers(self, names=None, register: bool = True) -> dict:
        """Host planes for filter_cloud_with_layers: one (rows, cols) Fortran-ordered float32 array per layer (Eigen::MatrixXf storage),
        registered with the context (gg_host_register) so that the device writes them directly -- what a host does once with the
        planes of its grid_map::GridMap."""
        names = list(LAYERS) if names is None else list(names)
        planes = {k: np.zeros((self.rows, self.cols), dtype=np.float32, order="F") for k in names}
        if register:
            for v in planes.values():
                _check(self._L, self._ctx, self._L.gg_host_register(self._ctx, v.ctypes.data, v.nbytes), "gg_host_register")
        return planes

    def release_layers(self, planes: dict):
        for v in planes.values():
            self._L.gg_host_unregister(self._ctx, v.ctypes.data)

    def filter_cloud_with_layers(self, cloud: np.ndarray, cloudOrigin: Sequence[float], mapToBase_z: float, planes: dict, map: Optional[GridMap] = None,
                                 return_details: bool = False, map_from_cloud=None, reuse_buffers: bool = False):
        """filter_cloud and the download of the layers in `planes` ({name: (rows, cols) F-ordered float32 array}) as ONE call
        (gg_filter_cloud_layers): what the reference's nodelet does per cloud -- filter, then publish every layer
        (src/GroundGridNodelet.cpp:196-228) -- with the layer traffic overlapping the terrain sweep."""
        assert cloud.dtype == POINT_DTYPE
        gm = map if map is not None else self._maps[0]
        cloud = np.ascontiguousarray(cloud)
        n = cloud.shape[0]
        out, labels, index = self._host_buffers(n, reuse_buffers)
        out_n = C.c_size_t(0)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        lab_p, idx_p = (labels.ctypes.data, index.ctypes.data) if return_details else (None, None)
        tf = None
        if map_from_cloud is not None:
            tf = (C.c_double * 12)(*[float(v) for v in np.asarray(map_from_cloud, dtype=np.float64).reshape(-1)[:12]])
        for k, v in planes.items():
            assert v.dtype == np.float32 and v.shape == (self.rows, self.cols) and v.flags.f_contiguous, k
        ptrs = (C.c_void_p * len(LAYERS))(*[planes[k].ctypes.data if k in planes else None for k in LAYERS])
        rc = self._L.gg_filter_cloud_layers(self._ctx, gm.slot, cloud.ctypes.data, n, tf, org, float(mapToBase_z), out.ctypes.data, C.byref(out_n),
                                            lab_p, idx_p, ptrs)
        _check(self._L, self._ctx, rc, "gg_filter_cloud_layers")
        seg = out[: out_n.value]
        if return_details:
            return seg, labels[:n], index[:n]
        return seg

    def filter_cloud_pc2(self, data: bytes, n: int, point_step: int, offsets, cloudOrigin, mapToBase_z: float,
                         map: Optional[GridMap] = None, map_from_cloud=None):
        """filter_cloud straight from a sensor_msgs/PointCloud2 payload; offsets = (x, y, z, ring) byte offsets.
        Returns (labels, out_index, n_returned) per input point."""
        gm = map if map is not None else self._maps[0]
        buf = np.frombuffer(data, dtype=np.uint8)
        assert buf.size >= n * point_step
        labels = np.zeros(max(n, 1), dtype=np.uint8)
        index = np.zeros(max(n, 1), dtype=np.int32)
        out_n = C.c_size_t(0)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        tf = None
        if map_from_cloud is not None:
            tf = (C.c_double * 12)(*[float(v) for v in np.asarray(map_from_cloud, dtype=np.float64).reshape(-1)[:12]])
        rc = self._L.gg_filter_cloud_pc2(self._ctx, gm.slot, buf.ctypes.data, n, point_step, offsets[0], offsets[1], offsets[2], offsets[3],
                                         tf, org, float(mapToBase_z), labels.ctypes.data, index.ctypes.data, C.byref(out_n))
        _check(self._L, self._ctx, rc, "gg_filter_cloud_pc2")
        return labels[:n], index[:n], out_n.value

    def filter_cloud_pc2_out(self, data: bytes, n: int, point_step: int, offsets, cloudOrigin, mapToBase_z: float,
                             map: Optional[GridMap] = None, map_from_cloud=None) -> np.ndarray:
        """PointCloud2 payload in, PointCloud2 payload out: the returned cloud as 18-byte records (x, y, z, intensity, ring --
        PC2_DTYPE), written by the label kernel.  Returns the structured array of the returned points."""
        gm = map if map is not None else self._maps[0]
        buf = np.frombuffer(data, dtype=np.uint8)
        assert buf.size >= n * point_step
        out = np.empty(max(n, 1) * _lib.GG_PC2_POINT_STEP, dtype=np.uint8)
        out_n = C.c_size_t(0)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        tf = None
        if map_from_cloud is not None:
            tf = (C.c_double * 12)(*[float(v) for v in np.asarray(map_from_cloud, dtype=np.float64).reshape(-1)[:12]])
        rc = self._L.gg_filter_cloud_pc2_out(self._ctx, gm.slot, buf.ctypes.data, n, point_step, offsets[0], offsets[1], offsets[2], offsets[3],
                                             tf, org, float(mapToBase_z), out.ctypes.data, C.byref(out_n))
        _check(self._L, self._ctx, rc, "gg_filter_cloud_pc2_out")
        return out[: out_n.value * _lib.GG_PC2_POINT_STEP].view(PC2_DTYPE)

    # -- insert_cloud's per-point decision (include/groundgrid/GroundSegmentation.h:55)
    def point_classes(self, n: int, map: Optional[GridMap] = None):
        gm = map if map is not None else self._maps[0]
        cls = np.zeros(max(n, 1), dtype=np.uint8)
        cell = np.zeros(max(n, 1), dtype=np.int32)
        rc = self._L.gg_get_point_classes(self._ctx, gm.slot, n, cls.ctypes.data, cell.ctypes.data)
        _check(self._L, self._ctx, rc, "gg_get_point_classes")
        return cls[:n], cell[:n]

    # -- batched device-resident form
    def filter_batch(self, points, n_points: Sequence[int], origins, base_z, *, first_slot: int = 0,
                     out: Optional[BatchOutputs] = None, want_clouds: bool = False, want_masks: bool = False, stream=None,
                     transforms=None, slots=None, want_pc2: bool = False, own_stream: bool = False) -> BatchOutputs:
        """points: CUDA torch tensor [B, stride, 16] (packed gg_point16) or [B, stride, 32] (PointXYZIR), uint8.
        Enqueues on the current torch stream and returns without synchronising.  own_stream: on the context's own stream instead (NULL in
        the C ABI): the caller makes sure that `points` is complete before the call."""
        import torch

        self._torch_used = True
        assert points.is_cuda and points.dtype == torch.uint8 and points.dim() == 3 and points.is_contiguous()
        B, stride, rec = points.shape
        assert rec in (16, 32)
        fmt = _lib.GG_POINT16 if rec == 16 else _lib.GG_POINT32
        if out is None:
            out = BatchOutputs(
                labels=torch.empty((B, stride), dtype=torch.uint8, device=points.device),
                out_index=torch.empty((B, stride), dtype=torch.int32, device=points.device),
                counts=torch.empty((B, 4), dtype=torch.int32, device=points.device),
                out_clouds=torch.empty((B, stride, 32), dtype=torch.uint8, device=points.device) if want_clouds else None,
                label_masks=torch.zeros((B, stride // 4), dtype=torch.uint8, device=points.device) if want_masks else None,
                out_pc2=torch.empty((B, stride * _lib.GG_PC2_POINT_STEP), dtype=torch.uint8, device=points.device) if want_pc2 else None,
            )
        npts = (C.c_int32 * B)(*[int(v) for v in n_points])
        org = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(B, 3))
        bz = np.ascontiguousarray(np.asarray(base_z, dtype=np.float64).reshape(B))
        b = GGBatch()
        b.n_clouds, b.first_slot, b.point_format = B, first_slot, fmt
        b.d_points, b.cloud_stride = points.data_ptr(), stride
        b.n_points = npts
        b.origins = org.ctypes.data_as(C.POINTER(C.c_float))
        b.base_z = bz.ctypes.data_as(C.POINTER(C.c_double))
        if transforms is not None:  # [B, 3, 4] map <- cloud frame: the per-point transform is fused into K1
            tfs = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(B, 12))
            b.transforms = tfs.ctypes.data_as(C.POINTER(C.c_double))
        if slots is not None:  # cloud b meets map slot slots[b] (distinct) instead of first_slot + b
            sl = (C.c_int32 * B)(*[int(v) for v in slots])
            b.slots = sl
        b.d_labels = out.labels.data_ptr()
        b.d_out_index = out.out_index.data_ptr()
        b.d_out_clouds = out.out_clouds.data_ptr() if out.out_clouds is not None else None
        b.d_out_counts = out.counts.data_ptr()
        b.d_label_masks = out.label_masks.data_ptr() if out.label_masks is not None else None
        b.d_out_pc2 = out.out_pc2.data_ptr() if out.out_pc2 is not None else None
        s = stream if stream is not None else torch.cuda.current_stream(points.device).cuda_stream
        # torch hands out 0 for its default stream = the legacy null stream; NULL would mean "the context's own stream" to
        # the library, which is not ordered with torch ops / RCCL -- so name the default stream explicitly
        rc = self._L.gg_filter_batch(self._ctx, C.byref(b), None if own_stream else C.c_void_p(s if s else _lib.GG_STREAM_DEFAULT))
        _check(self._L, self._ctx, rc, "gg_filter_batch")
        return out

    def batch_fence(self, stream=None):
        """GG_FLAG_CONCURRENT_HALVES: order the current torch stream (or `stream`) after both halves of the batches enqueued so far --
        before anything the caller enqueues itself reads their outputs."""
        _check(self._L, self._ctx, self._L.gg_batch_fence(self._ctx, self._stream_arg(True, handle=stream)), "gg_batch_fence")

    def kernel_times(self, reset: bool = True):
        """(ms[7], launches[7]) accumulated under set_flags(profile=True)."""
        ms = (C.c_double * _lib.GG_NUM_KERNELS)()
        ln = (C.c_int64 * _lib.GG_NUM_KERNELS)()
        _check(self._L, self._ctx, self._L.gg_get_kernel_times(self._ctx, ms, ln, 1 if reset else 0), "gg_get_kernel_times")
        names = [self._L.gg_kernel_name(k).decode() for k in range(_lib.GG_NUM_KERNELS)]
        return {names[k]: (ms[k], ln[k]) for k in range(_lib.GG_NUM_KERNELS)}

    def synchronize(self):
        """Waits for everything the context has enqueued, batches on caller streams included (the library orders its own
        stream after them, include/groundgrid_hip.h gg_filter_batch)."""
        _check(self._L, self._ctx, self._L.gg_synchronize(self._ctx), "gg_synchronize")

    # -- pipelined reference-shaped call (gg_filter_cloud_async / gg_filter_cloud_wait)
    def filter_cloud_async(self, cloud: np.ndarray, cloudOrigin: Sequence[float], mapToBase_z: float, map: Optional[GridMap] = None,
                           map_from_cloud=None) -> int:
        """Enqueue one cloud and return a ticket; at most GG_ASYNC_DEPTH tickets may be outstanding."""
        assert cloud.dtype == POINT_DTYPE
        gm = map if map is not None else self._maps[0]
        cloud = np.ascontiguousarray(cloud)
        org = (C.c_float * 3)(*[float(v) for v in cloudOrigin])
        tf = None
        if map_from_cloud is not None:
            tf = (C.c_double * 12)(*[float(v) for v in np.asarray(map_from_cloud, dtype=np.float64).reshape(-1)[:12]])
        t = C.c_int(-1)
        rc = self._L.gg_filter_cloud_async(self._ctx, gm.slot, cloud.ctypes.data, cloud.shape[0], tf, org, float(mapToBase_z), C.byref(t))
        _check(self._L, self._ctx, rc, "gg_filter_cloud_async")
        self._async[t.value] = cloud  # keeps the input alive until the wait
        return t.value

    def filter_cloud_wait(self, ticket: int, return_details: bool = False, want_cloud: bool = True, reuse_buffers: bool = False):
        cloud = self._async.pop(ticket)
        n = cloud.shape[0]
        out, labels, index = self._host_buffers(n, reuse_buffers)
        if not want_cloud:
            out = None
        out_n = C.c_size_t(0)
        rc = self._L.gg_filter_cloud_wait(self._ctx, ticket, out.ctypes.data if want_cloud else None, C.byref(out_n),
                                          labels.ctypes.data if return_details else None, index.ctypes.data if return_details else None)
        _check(self._L, self._ctx, rc, "gg_filter_cloud_wait")
        seg = out[: out_n.value] if want_cloud else None
        if return_details:
            return seg, labels[:n], index[:n]
        return seg

    def debug_set_tuning(self, key: str, value: int) -> int:
        """Tools / tests: force a launch geometry the library would otherwise derive from the batch size ("sweep_waves",
        "k2_per_cloud", "k2_dense_share"; 0 = default); key "pw" returns the context's points per wave chunk."""
        fn = self._L.gg_debug_set_tuning
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        rc = fn(self._ctx, key.encode(), int(value))
        if rc < 0:
            raise GroundGridError(f"gg_debug_set_tuning({key}): {_lib.STATUS.get(rc, rc)}")
        return rc

    def debug_regions_tile(self, value: int = -1) -> int:
        """Tools / tests: which path cluster_planes takes (gg_debug_regions_tile): 1 = 32 x 32 tiles labelled in LDS in front of the
        flatten, 0 = the plain merge; the same results.  A negative value changes nothing.  Returns the path the library ships with."""
        fn = self._L.gg_debug_regions_tile
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int]
        rc = fn(self._ctx, int(value))
        if rc < 0:
            raise GroundGridError(f"gg_debug_regions_tile: {_lib.STATUS.get(rc, rc)}")
        return rc

    def set_conventions(self, eigen_reduction: int = 0):
        """Which Eigen the reference is built against (0 = 3.3.x order of the 5x5 block sums, 1 = 3.4.x SSE2)."""
        c = _lib.GGConventions()
        c.eigen_reduction = int(eigen_reduction)
        _check(self._L, self._ctx, self._L.gg_set_conventions(self._ctx, C.byref(c)), "gg_set_conventions")
