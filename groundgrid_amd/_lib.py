"""ctypes loader for libgroundgrid_hip.so (the C ABI of include/groundgrid_hip.h).

The library is built in-tree by ``groundgrid_amd.build.build()`` (hipcc, gfx950).  Loading fails loudly
if the .so is missing: the product has no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GROUNDGRID_HIP_LIB") or os.path.join(_HERE, "libgroundgrid_hip.so")  # override: side-by-side builds

GG_OK = 0
STATUS = {
    0: "GG_OK",
    -1: "GG_ERR_INVALID",
    -2: "GG_ERR_GEOMETRY",
    -3: "GG_ERR_NOMEM",
    -4: "GG_ERR_HIP",
    -5: "GG_ERR_CAPACITY",
    -6: "GG_ERR_NO_DEVICE",
}

GG_ABI_VERSION = 6  # include/groundgrid_hip.h
GG_POINT32, GG_POINT16 = 0, 1
GG_FLAG_MINIMAL_LAYERS, GG_FLAG_PROFILE, GG_FLAG_CONCURRENT_HALVES, GG_FLAG_EAGER_LAYERS = 1, 2, 4, 8
GG_NUM_KERNELS = 7
GG_NUM_LAYERS = 11

LAYERS = [
    "points", "ground", "groundpatch", "minGroundHeight", "maxGroundHeight", "groundCandidates",
    "planeDist", "m2", "meanVariance", "pointsRaw", "variance",
]

# every symbol include/groundgrid_hip.h declares
SYMBOLS = [
    "gg_abi_version", "gg_kernel_name", "gg_default_config", "gg_default_geometry", "gg_create", "gg_destroy",
    "gg_set_config", "gg_get_config", "gg_set_slot_configs", "gg_get_slot_config", "gg_set_flags", "gg_get_size", "gg_get_geometry", "gg_last_error",
    "gg_reset_map", "gg_reset_maps", "gg_set_map_position", "gg_move_map", "gg_move_maps", "gg_get_map_position", "gg_set_layer", "gg_get_layer", "gg_get_layers", "gg_get_expected_points",
    "gg_filter_cloud", "gg_filter_cloud_tf", "gg_filter_cloud_pc2", "gg_get_layer_image_u8", "gg_get_terrain_image", "gg_filter_batch", "gg_synchronize", "gg_get_point_classes", "gg_get_kernel_times",
    "gg_set_conventions", "gg_get_conventions", "gg_rotation_from_quaternion", "gg_transform_from_pose",
    "gg_filter_cloud_async", "gg_filter_cloud_wait", "gg_debug_emulate_ring_sweep", "gg_debug_sweep_sync_selftest",
    "gg_batch_fence", "gg_device_error", "gg_filter_cloud_layers", "gg_host_register", "gg_host_unregister", "gg_run_stage", "gg_insert_cloud", "gg_filter_cloud_pc2_out", "gg_get_gridmap_message",
    "gg_collective_available", "gg_comm_unique_id", "gg_comm_init_rank", "gg_comm_init_rank_for", "gg_comm_destroy", "gg_allgather_label_masks",
    "gg_set_score_labels", "gg_set_slot_scoring", "gg_get_slot_scores", "gg_reset_slot_scores", "gg_get_score_kernel_time",
    "gg_export_layers",
    "gg_import_layers",
    "gg_export_images",
    "gg_split_clouds",
    "gg_rasterize_clouds",
    "gg_export_slopes",
    "gg_cluster_clouds",
    "gg_clearance_clouds",
    "gg_visibility_clouds",
    "gg_fuse_states",
    "gg_route_planes",
    "gg_match_planes",
    "gg_footprint_planes",
    "gg_footprint_spans",
    "gg_route_headings",
    "gg_heading_moves",
    "gg_track_clusters",
    "gg_box_clusters",
    "gg_score_rollouts",
    "gg_cluster_planes",
]

GG_EIGEN_33, GG_EIGEN_34_SSE = 0, 1
GG_PLANES_COLMAJOR, GG_PLANES_ROWMAJOR = 0, 1
# gg_rasterize_clouds: the channels in GG_RASTER_* order (a channel's bit of channel_mask is its position here)
RASTER_CHANNELS = ("nonground_count", "nonground_max_height", "nonground_min_height", "ground_count", "ground_max_height", "ground_min_height")
(GG_RASTER_NONGROUND_COUNT, GG_RASTER_NONGROUND_MAX_HEIGHT, GG_RASTER_NONGROUND_MIN_HEIGHT, GG_RASTER_GROUND_COUNT, GG_RASTER_GROUND_MAX_HEIGHT,
 GG_RASTER_GROUND_MIN_HEIGHT) = range(6)
GG_NUM_RASTER_CHANNELS = 6
# gg_export_slopes: the channels in GG_SLOPE_* order (a channel's bit of channel_mask is its position here)
SLOPE_CHANNELS = ["grad_x", "grad_y", "tangent", "normal_z", "step", "min_confidence"]
GG_SLOPE_GRAD_X, GG_SLOPE_GRAD_Y, GG_SLOPE_TANGENT, GG_SLOPE_NORMAL_Z, GG_SLOPE_STEP, GG_SLOPE_MIN_CONFIDENCE = range(6)
GG_NUM_SLOPE_CHANNELS = 6
GG_TERRAIN_HWC, GG_TERRAIN_CHW = 0, 1
GG_ROT_TF2, GG_ROT_KDL = 0, 1
ROTATION = {"tf2": GG_ROT_TF2, "kdl": GG_ROT_KDL}
GG_ASYNC_DEPTH = 2
GG_STREAM_DEFAULT = C.c_void_p(-1).value  # include/groundgrid_hip.h: the legacy default ("null") stream -- what torch's handle 0 means


class GGConfig(C.Structure):
    """gg_config == groundgrid::GroundGridConfig (cfg/GroundGrid.cfg:8-21)"""

    _fields_ = [
        ("point_count_cell_variance_threshold", C.c_int),
        ("max_ring", C.c_int),
        ("groundpatch_detection_minimum_threshold", C.c_double),
        ("distance_factor", C.c_double),
        ("minimum_distance_factor", C.c_double),
        ("miminum_point_height_threshold", C.c_double),
        ("minimum_point_height_obstacle_threshold", C.c_double),
        ("outlier_tolerance", C.c_double),
        ("ground_patch_detection_minimum_point_count_threshold", C.c_double),
        ("patch_size_change_distance", C.c_double),
        ("occupied_cells_decrease_factor", C.c_double),
        ("occupied_cells_point_count_factor", C.c_double),
        ("min_outlier_detection_ground_confidence", C.c_double),
        ("thread_count", C.c_int),
    ]


class GGConventions(C.Structure):
    _fields_ = [("eigen_reduction", C.c_int), ("reserved", C.c_int * 7)]


class GGGeometry(C.Structure):
    _fields_ = [
        ("length", C.c_float),
        ("resolution", C.c_float),
        ("vertical_point_ang_dist", C.c_float),
        ("min_dist_squared", C.c_float),
    ]


class GGBatch(C.Structure):
    _fields_ = [
        ("n_clouds", C.c_int),
        ("first_slot", C.c_int),
        ("point_format", C.c_int),
        ("d_points", C.c_void_p),
        ("cloud_stride", C.c_size_t),
        ("n_points", C.POINTER(C.c_int32)),
        ("origins", C.POINTER(C.c_float)),
        ("base_z", C.POINTER(C.c_double)),
        ("transforms", C.POINTER(C.c_double)),
        ("d_labels", C.c_void_p),
        ("d_out_index", C.c_void_p),
        ("d_out_clouds", C.c_void_p),
        ("d_out_counts", C.c_void_p),
        ("d_label_masks", C.c_void_p),
        ("slots", C.POINTER(C.c_int32)),
        ("d_out_pc2", C.c_void_p),
    ]


class GGImageExport(C.Structure):
    """gg_image_export: the u8 layer images and the terrain images of many maps, in device memory (gg_export_images)"""

    _fields_ = [
        ("n", C.c_int),
        ("first_slot", C.c_int),
        ("slots", C.POINTER(C.c_int32)),
        ("layer_mask", C.c_uint),
        ("d_images", C.c_void_p),
        ("image_stride", C.c_size_t),
        ("d_bounds", C.c_void_p),
        ("d_terrain", C.c_void_p),
        ("terrain_stride", C.c_size_t),
        ("terrain_layout", C.c_int),
    ]


class GGSplitSet(C.Structure):
    """gg_split_set: one selected set of every cloud (gg_split_clouds); each pointer nullable"""

    _fields_ = [("d_points", C.c_void_p), ("d_height", C.c_void_p), ("d_source", C.c_void_p)]


# the labelled clouds of a call: the ten leading members of gg_cloud_split, gg_cloud_raster, gg_cloud_clusters, gg_cloud_clearance and
# gg_cloud_visibility
_LABELLED_CLOUDS = [
    ("n", C.c_int),
    ("first_slot", C.c_int),
    ("slots", C.POINTER(C.c_int32)),
    ("point_format", C.c_int),
    ("d_points", C.c_void_p),
    ("cloud_stride", C.c_size_t),
    ("n_points", C.POINTER(C.c_int32)),
    ("transforms", C.POINTER(C.c_double)),
    ("d_labels", C.c_void_p),
    ("d_label_masks", C.c_void_p),
]


class GGCloudSplit(C.Structure):
    """gg_cloud_split: the ground and the non-ground points of many labelled clouds as dense clouds, in device memory (gg_split_clouds)"""

    _fields_ = _LABELLED_CLOUDS + [
        ("ground", GGSplitSet),
        ("nonground", GGSplitSet),
        ("d_counts", C.c_void_p),
    ]


class GGCloudRaster(C.Structure):
    """gg_cloud_raster: the obstacle grid of many labelled clouds as dense planes, in device memory (gg_rasterize_clouds)"""

    _fields_ = _LABELLED_CLOUDS + [
        ("channel_mask", C.c_uint),
        ("order", C.c_int),
        ("d_dst", C.c_void_p),
        ("plane_stride", C.c_size_t),
    ]


class GGCluster(C.Structure):
    """gg_cluster: one obstacle cluster of a cloud (gg_cluster_clouds), 32 bytes"""

    _fields_ = [
        ("cells", C.c_int32),
        ("points", C.c_int32),
        ("row_min", C.c_int32),
        ("row_max", C.c_int32),
        ("col_min", C.c_int32),
        ("col_max", C.c_int32),
        ("height_max", C.c_float),
        ("first_cell", C.c_int32),
    ]


class GGCloudClusters(C.Structure):
    """gg_cloud_clusters: the obstacle clusters of many labelled clouds, in device memory (gg_cluster_clouds)"""

    _fields_ = _LABELLED_CLOUDS + [
        ("min_points", C.c_int),
        ("min_height", C.c_float),
        ("max_height", C.c_float),
        ("connectivity", C.c_int),
        ("order", C.c_int),
        ("d_cell_cluster", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_point_cluster", C.c_void_p),
        ("d_n_clusters", C.c_void_p),
        ("d_clusters", C.c_void_p),
        ("max_clusters", C.c_int),
    ]


GG_CLEARANCE_NONE = 0x7FFFFFFF  # d_dist2 of a cell without an obstacle (an empty map, or beyond max_cells)


class GGCloudClearance(C.Structure):
    """gg_cloud_clearance: the obstacle distance field of many maps, in device memory (gg_clearance_clouds)"""

    _fields_ = _LABELLED_CLOUDS + [
        ("min_points", C.c_int),
        ("min_height", C.c_float),
        ("max_height", C.c_float),
        ("d_seeds", C.c_void_p),
        ("seed_stride", C.c_size_t),
        ("max_cells", C.c_int),
        ("order", C.c_int),
        ("d_dist2", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_nearest", C.c_void_p),
        ("d_distance", C.c_void_p),
        ("d_n_occupied", C.c_void_p),
    ]


GG_CELL_FREE, GG_CELL_UNKNOWN, GG_CELL_OCCUPIED = -1, 0, 1  # the states of a d_state plane (gg_visibility_clouds)


class GGCloudVisibility(C.Structure):
    """gg_cloud_visibility: the free, unknown and occupied cells of many labelled clouds, in device memory (gg_visibility_clouds)"""

    _fields_ = _LABELLED_CLOUDS + [
        ("min_points", C.c_int),
        ("min_height", C.c_float),
        ("max_height", C.c_float),
        ("origins", C.POINTER(C.c_float)),
        ("max_cells", C.c_int),
        ("order", C.c_int),
        ("d_state", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_counts", C.c_void_p),
    ]


class GGStateFusion(C.Structure):
    """gg_state_fusion: the evidence, fused state and frontier planes of many maps carried from scan to scan (gg_fuse_states)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_state", C.c_void_p),
        ("state_stride", C.c_size_t),
        ("d_evidence_in", C.c_void_p),
        ("shifts", C.POINTER(C.c_int32)),
        ("hit", C.c_int),
        ("miss", C.c_int),
        ("decay", C.c_int),
        ("e_min", C.c_int),
        ("e_max", C.c_int),
        ("free_threshold", C.c_int),
        ("occ_threshold", C.c_int),
        ("order", C.c_int),
        ("d_evidence_out", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_fused", C.c_void_p),
        ("d_frontier", C.c_void_p),
        ("d_counts", C.c_void_p),
    ]


GG_FUSE_LIMIT = (1 << 30) - 1  # the largest hit, miss, decay, -e_min and e_max of gg_fuse_states
# the cells a work-group of k18_fuse.hip owns, along the contiguous direction of `order` and across it (gg_internal.h FUSE_TILE_X / _Y):
# where the tests of the frontier put their tile seams
GG_FUSE_TILE = (62, 26)


class GGPlaneRoutes(C.Structure):
    """gg_plane_routes: the cost-to-go, next-cell and path outputs of many maps over caller-given goal, blocked and cost planes (gg_route_planes)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_blocked", C.c_void_p),
        ("blocked_stride", C.c_size_t),
        ("d_cost", C.c_void_p),
        ("cost_stride", C.c_size_t),
        ("d_goals", C.c_void_p),
        ("goal_stride", C.c_size_t),
        ("connectivity", C.c_int),
        ("straight", C.c_int),
        ("diagonal", C.c_int),
        ("cost_max", C.c_int),
        ("max_cost", C.c_int),
        ("order", C.c_int),
        ("d_dist", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_next", C.c_void_p),
        ("d_counts", C.c_void_p),
        ("starts", C.POINTER(C.c_int32)),
        ("d_paths", C.c_void_p),
        ("max_path", C.c_int),
        ("d_path_len", C.c_void_p),
    ]


GG_ROUTE_NONE = 0x7FFFFFFF  # d_dist of a cell no admissible path leads from (gg_route_planes)
GG_HAS_ROUTE_PLANES = 1
GG_ROUTE_LIMIT = (1 << 31) - 2  # the largest max(straight, diagonal) * cost_max * rows * cols of gg_route_planes
# the side of the tiles a work-group of k19_route.hip relaxes a map by (gg_internal.h ROUTE_TILE): where the tests put their tile seams
GG_ROUTE_TILE = 64


class GGPlaneMatches(C.Structure):
    """gg_plane_matches: the best alignment (yaw candidate, translation) of many scan planes to their field planes (gg_match_planes)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_scan", C.c_void_p),
        ("scan_stride", C.c_size_t),
        ("d_field", C.c_void_p),
        ("field_stride", C.c_size_t),
        ("field_max", C.c_int),
        ("shifts", C.POINTER(C.c_int32)),
        ("pivots", C.POINTER(C.c_int32)),
        ("rotations", C.POINTER(C.c_int32)),
        ("n_rotations", C.c_int),
        ("window", C.c_int),
        ("order", C.c_int),
        ("d_best", C.c_void_p),
        ("d_scores", C.c_void_p),
        ("score_stride", C.c_size_t),
    ]


GG_HAS_MATCH_PLANES = 1
GG_MATCH_MAX_WINDOW = 32      # the largest `window` of gg_match_planes
GG_MATCH_MAX_ROTATIONS = 64   # ... and the most yaw candidates
GG_MATCH_UNIT = 16384         # 1.0 of a rotation pair (Q14)
GG_MATCH_LIMIT = (1 << 31) - 1  # the largest field_max * rows * cols
GG_MATCH_MAX_SIDE = 32768     # more rows or cols is GG_ERR_GEOMETRY
# the cells of the scan plane a work-group of k20_match.hip looks at between two barriers, and the entries of its list (MATCH_CHUNK,
# MATCH_LIST): where the tests put their chunk seams and how many scan cells fill the list
GG_MATCH_CHUNK = 1024
GG_MATCH_LIST = 2048


class GGPlaneFootprints(C.Structure):
    """gg_plane_footprints: which headings of a footprint fit at every cell of many blocked planes (gg_footprint_planes)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_blocked", C.c_void_p),
        ("blocked_stride", C.c_size_t),
        ("spans", C.POINTER(C.c_int32)),
        ("n_headings", C.c_int),
        ("radius", C.c_int),
        ("min_fit", C.c_int),
        ("outside_free", C.c_int),
        ("order", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_stride", C.c_size_t),
        ("d_fit", C.c_void_p),
        ("fit_stride", C.c_size_t),
        ("d_counts", C.c_void_p),
    ]


GG_HAS_FOOTPRINT_PLANES = 1
GG_FOOTPRINT_MAX_HEADINGS = 32  # the most headings of gg_footprint_planes
GG_FOOTPRINT_MAX_RADIUS = 32    # ... and its largest radius
GG_FOOTPRINT_RECT_LIMIT = 1 << 30  # the largest |word| of the rectangle of gg_footprint_spans
# the side of a work-group's tile in k21_footprint.hip (FOOTPRINT_TILE): where the tests put their seams
GG_FOOTPRINT_TILE = 64


class GGHeadingRoutes(C.Structure):
    """gg_heading_routes: the cost-to-go over cells and headings, the moves and the paths of many maps over a heading mask (gg_route_headings)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_stride", C.c_size_t),
        ("d_cost", C.c_void_p),
        ("cost_stride", C.c_size_t),
        ("d_goals", C.c_void_p),
        ("goal_stride", C.c_size_t),
        ("goal_headings", C.c_uint32),
        ("n_headings", C.c_int),
        ("moves", C.POINTER(C.c_int32)),
        ("cost_max", C.c_int),
        ("max_cost", C.c_int),
        ("order", C.c_int),
        ("d_dist", C.c_void_p),
        ("dist_stride", C.c_size_t),
        ("plane_stride", C.c_size_t),
        ("d_next", C.c_void_p),
        ("next_stride", C.c_size_t),
        ("next_plane_stride", C.c_size_t),
        ("d_best", C.c_void_p),
        ("best_stride", C.c_size_t),
        ("d_best_heading", C.c_void_p),
        ("best_heading_stride", C.c_size_t),
        ("d_counts", C.c_void_p),
        ("starts", C.POINTER(C.c_int32)),
        ("d_paths", C.c_void_p),
        ("path_stride", C.c_size_t),
        ("max_len", C.c_int),
        ("d_path_len", C.c_void_p),
    ]


GG_HAS_ROUTE_HEADINGS = 1
GG_HEADINGS_MAX = 32         # the most headings of gg_route_headings
GG_HEADINGS_MAX_MOVES = 8    # ... moves per heading
GG_HEADINGS_MAX_STEP = 3     # ... cells a move spans along either axis
GG_HEADINGS_MAX_COST = 32767  # ... and the largest cost s of a move
GG_HEADINGS_AT_GOAL = 8      # d_next of a goal state
GG_HEADINGS_LIMIT = (1 << 31) - 2  # the largest max s * cost_max * rows * cols * n_headings


def headings_tile(n_headings):
    """the side of the tiles a work-group of k22_headings.hip relaxes a map by (gg_internal.h headings_tile): where the tests put their seams"""
    return 32 if n_headings <= 16 else 16


class GGTrack(C.Structure):
    """gg_track: record k of a map describes cluster k of this scan (gg_track_clusters)"""

    _fields_ = [
        ("track_id", C.c_int32),
        ("age", C.c_int32),
        ("prev", C.c_int32),
        ("overlap", C.c_int32),
        ("still", C.c_int32),
        ("cells", C.c_int32),
        ("sum_row", C.c_int32),
        ("sum_col", C.c_int32),
    ]


class GGClusterTracks(C.Structure):
    """gg_cluster_tracks: this scan's clusters of many maps associated with the last scan's (gg_track_clusters)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_cells", C.c_void_p),
        ("cells_stride", C.c_size_t),
        ("d_cells_prev", C.c_void_p),
        ("prev_stride", C.c_size_t),
        ("d_tracks_in", C.c_void_p),
        ("d_heads_in", C.c_void_p),
        ("shifts", C.POINTER(C.c_int32)),
        ("max_clusters", C.c_int),
        ("gate", C.c_int),
        ("order", C.c_int),
        ("d_tracks_out", C.c_void_p),
        ("d_heads_out", C.c_void_p),
        ("d_cell_track", C.c_void_p),
        ("track_stride", C.c_size_t),
    ]


GG_HAS_TRACK_CLUSTERS = 1
GG_TRACK_MAX_CLUSTERS = 1024  # the most clusters per map of gg_track_clusters
GG_TRACK_MAX_GATE = 4         # ... and its widest gate, in cells
# the words of the contingency matrix a work-group of k23_tracks.hip holds at a time (gg_internal.h TRACK_SLAB_WORDS): with more than
# TRACK_SLAB_WORDS / Kp current clusters the plane is walked once per slab, which is where the tests put their cluster counts
GG_TRACK_SLAB_WORDS = 28 * 1024


class GGBox(C.Structure):
    """gg_box: record c of a cloud is the oriented box of its cluster c (gg_box_clusters), 32 bytes"""

    _fields_ = [
        ("heading", C.c_int32),
        ("points", C.c_int32),
        ("a_min", C.c_int32),
        ("a_max", C.c_int32),
        ("b_min", C.c_int32),
        ("b_max", C.c_int32),
        ("cost_lo", C.c_int32),
        ("cost_hi", C.c_int32),
    ]


class GGClusterBoxes(C.Structure):
    """gg_cluster_boxes: the oriented boxes of the obstacle clusters of many clouds, in device memory (gg_box_clusters)"""

    _fields_ = _LABELLED_CLOUDS[:8] + [
        ("d_point_cluster", C.c_void_p),
        ("d_n_clusters", C.c_void_p),
        ("rotations", C.POINTER(C.c_int32)),
        ("n_rotations", C.c_int),
        ("criterion", C.c_int),
        ("max_clusters", C.c_int),
        ("d_boxes", C.c_void_p),
        ("d_costs", C.c_void_p),
    ]


GG_HAS_BOX_CLUSTERS = 1
GG_BOX_UNIT = 16              # units per cell of gg_box_clusters' quantisation
GG_BOX_MAX_HEADINGS = 32      # the most candidate headings of a call
GG_BOX_MAX_CLUSTERS = 4096    # ... and the most clusters per cloud
GG_BOX_AREA, GG_BOX_EDGE = 0, 1
BOX_CRITERIA = ("area", "edge")
# the bytes of LDS a work-group of k24_boxes.hip fills with clusters at a time (gg_internal.h BOX_LDS_BUDGET): 24 per (cluster, heading) and
# 4 per cluster; with more clusters the ids are walked once per slab, which is where the tests put their cluster counts
GG_BOX_LDS_BUDGET = 144 * 1024


def box_slab_clusters(n_headings: int, max_clusters: int) -> int:
    """the clusters a work-group of k24_boxes.hip holds at a time (gg_internal.h box_slab_clusters)"""
    return min(max_clusters, GG_BOX_LDS_BUDGET // (24 * n_headings + 4))


class GGRollouts(C.Structure):
    """gg_rollouts: the scores of candidate trajectories of many maps over the planes of the device chain (gg_score_rollouts)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_stride", C.c_size_t),
        ("d_cost", C.c_void_p),
        ("cost_stride", C.c_size_t),
        ("d_dist", C.c_void_p),
        ("dist_stride", C.c_size_t),
        ("plane_stride", C.c_size_t),
        ("d_clear", C.c_void_p),
        ("clear_stride", C.c_size_t),
        ("n_headings", C.c_int),
        ("starts", C.POINTER(C.c_int32)),
        ("rotations", C.POINTER(C.c_int32)),
        ("frame", C.c_int),
        ("d_table", C.c_void_p),
        ("table_stride", C.c_size_t),
        ("n_rollouts", C.c_int),
        ("n_steps", C.c_int),
        ("cost_max", C.c_int),
        ("reach", C.c_int),
        ("order", C.c_int),
        ("d_records", C.c_void_p),
        ("record_stride", C.c_size_t),
        ("d_best", C.c_void_p),
    ]


GG_HAS_SCORE_ROLLOUTS = 1
GG_ROLLOUTS_MAX = 65536        # the most rollouts per map of gg_score_rollouts
GG_ROLLOUTS_MAX_STEPS = 128    # ... steps per rollout
GG_ROLLOUTS_MAX_REACH = 63     # ... and the widest reach, in cells
GG_ROLLOUTS_RECORD_WORDS = 8   # words of a record
GG_ROLLOUTS_RELATIVE, GG_ROLLOUTS_ABSOLUTE = 0, 1
GG_ROLLOUTS_LIMIT = (1 << 31) - 2  # the largest n_steps * 32767 * cost_max


class GGRegion(C.Structure):
    """gg_region: record k of a map describes its kept component k (gg_cluster_planes), 48 bytes"""

    _fields_ = [
        ("cells", C.c_int32),
        ("row_min", C.c_int32),
        ("row_max", C.c_int32),
        ("col_min", C.c_int32),
        ("col_max", C.c_int32),
        ("first_cell", C.c_int32),
        ("value_cell", C.c_int32),
        ("value_min", C.c_int32),
        ("sum_row", C.c_int64),
        ("sum_col", C.c_int64),
    ]


class GGPlaneClusters(C.Structure):
    """gg_plane_clusters: the connected regions of any int32 plane of many maps, in device memory (gg_cluster_planes)"""

    _fields_ = [
        ("n", C.c_int),
        ("d_seeds", C.c_void_p),
        ("seed_stride", C.c_size_t),
        ("lo", C.c_int32),
        ("hi", C.c_int32),
        ("connectivity", C.c_int),
        ("min_cells", C.c_int),
        ("order", C.c_int),
        ("d_values", C.c_void_p),
        ("value_stride", C.c_size_t),
        ("d_cell_cluster", C.c_void_p),
        ("plane_stride", C.c_size_t),
        ("d_cell_size", C.c_void_p),
        ("size_stride", C.c_size_t),
        ("d_heads", C.c_void_p),
        ("d_regions", C.c_void_p),
        ("max_regions", C.c_int),
    ]


GG_HAS_CLUSTER_PLANES = 1
GG_REGION_BYTES = 48           # sizeof(gg_region)


GG_PC2_POINT_STEP = 18
GG_SCORE_MAX_LABELS = 64


class GGSlotScores(C.Structure):
    """gg_slot_scores: counts[bin][0] = predicted non-ground, [bin][1] = predicted ground; bin n_ids = every id that is not listed"""

    _fields_ = [("clouds", C.c_uint64), ("counts", (C.c_uint64 * 2) * (GG_SCORE_MAX_LABELS + 1))]


GG_STAGE_DETECT_GROUND_PATCHES, GG_STAGE_SPIRAL_GROUND_INTERPOLATION = 1, 2
GG_STAGE_DETECT_GROUND_PATCH_3, GG_STAGE_DETECT_GROUND_PATCH_5, GG_STAGE_INTERPOLATE_CELL = 3, 4, 5


class GGStageArgs(C.Structure):
    _fields_ = [("section", C.c_int), ("i", C.c_int), ("j", C.c_int), ("base_z", C.c_double)]


class GGGridMapHeader(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("frame_id", C.c_char_p), ("basic_layers", C.c_uint)]


class GroundGridError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GroundGridError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp = C.c_void_p
    L.gg_abi_version.restype = C.c_int
    if L.gg_abi_version() != GG_ABI_VERSION:  # (struct layouts below are this version's: a stale .so would read past gg_batch)
        raise GroundGridError(f"{LIB_PATH} has ABI version {L.gg_abi_version()}, this package expects {GG_ABI_VERSION}: rebuild it")
    L.gg_kernel_name.restype = C.c_char_p
    L.gg_kernel_name.argtypes = [C.c_int]
    L.gg_default_config.argtypes = [P(GGConfig)]
    L.gg_default_config.restype = None
    L.gg_default_geometry.argtypes = [P(GGGeometry)]
    L.gg_default_geometry.restype = None
    L.gg_create.argtypes = [P(GGGeometry), C.c_int, C.c_size_t, C.c_int, P(vp)]
    L.gg_destroy.argtypes = [vp]
    L.gg_destroy.restype = None
    L.gg_set_config.argtypes = [vp, P(GGConfig)]
    L.gg_get_config.argtypes = [vp, P(GGConfig)]
    L.gg_set_slot_configs.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, P(GGConfig)]
    L.gg_get_slot_config.argtypes = [vp, C.c_int, P(GGConfig), P(C.c_int)]
    L.gg_set_flags.argtypes = [vp, C.c_uint]
    L.gg_get_size.argtypes = [vp, P(C.c_int), P(C.c_int)]
    L.gg_get_geometry.argtypes = [vp, P(C.c_double), P(C.c_double), P(C.c_double)]
    L.gg_last_error.argtypes = [vp]
    L.gg_last_error.restype = C.c_char_p
    L.gg_reset_map.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_float]
    L.gg_reset_maps.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float, C.c_int, vp]
    L.gg_set_map_position.argtypes = [vp, C.c_int, C.c_double, C.c_double]
    L.gg_move_map.argtypes = [vp, C.c_int, C.c_double, C.c_double, P(C.c_double), P(C.c_int)]
    L.gg_move_maps.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, P(C.c_double), P(C.c_double), P(C.c_int32), vp]
    L.gg_export_layers.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, C.c_uint, C.c_int, vp, C.c_size_t, vp]
    L.gg_import_layers.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, C.c_uint, C.c_int, vp, C.c_size_t, vp]
    L.gg_export_images.argtypes = [vp, P(GGImageExport), vp]
    L.gg_split_clouds.argtypes = [vp, P(GGCloudSplit), vp]
    L.gg_rasterize_clouds.argtypes = [vp, P(GGCloudRaster), vp]
    L.gg_export_slopes.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, C.c_uint, C.c_int, vp, C.c_size_t, vp]
    L.gg_cluster_clouds.argtypes = [vp, P(GGCloudClusters), vp]
    L.gg_clearance_clouds.argtypes = [vp, P(GGCloudClearance), vp]
    L.gg_visibility_clouds.argtypes = [vp, P(GGCloudVisibility), vp]
    L.gg_fuse_states.argtypes = [vp, P(GGStateFusion), vp]
    L.gg_route_planes.argtypes = [vp, P(GGPlaneRoutes), vp]
    L.gg_match_planes.argtypes = [vp, P(GGPlaneMatches), vp]
    L.gg_footprint_planes.argtypes = [vp, P(GGPlaneFootprints), vp]
    L.gg_footprint_spans.argtypes = [P(C.c_int32), C.c_int, P(C.c_int32), C.c_int, P(C.c_int32), P(C.c_int)]
    L.gg_route_headings.argtypes = [vp, P(GGHeadingRoutes), vp]
    L.gg_heading_moves.argtypes = [P(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int32)]
    L.gg_track_clusters.argtypes = [vp, P(GGClusterTracks), vp]
    L.gg_box_clusters.argtypes = [vp, P(GGClusterBoxes), vp]
    L.gg_score_rollouts.argtypes = [vp, P(GGRollouts), vp]
    L.gg_cluster_planes.argtypes = [vp, P(GGPlaneClusters), vp]
    L.gg_get_map_position.argtypes =[vp, C.c_int, P(C.c_double), P(C.c_double)]
    L.gg_set_layer.argtypes = [vp, C.c_int, C.c_int, vp]
    L.gg_get_layer.argtypes = [vp, C.c_int, C.c_int, vp]
    L.gg_get_expected_points.argtypes = [vp, vp]
    L.gg_filter_cloud.argtypes = [vp, C.c_int, vp, C.c_size_t, P(C.c_float), C.c_double, vp, P(C.c_size_t), vp, vp]
    L.gg_filter_cloud_tf.argtypes = [vp, C.c_int, vp, C.c_size_t, P(C.c_double), P(C.c_float), C.c_double, vp, P(C.c_size_t), vp, vp]
    L.gg_filter_cloud_pc2.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, P(C.c_double), P(C.c_float), C.c_double, vp, vp, P(C.c_size_t)]
    L.gg_get_layers.argtypes = [vp, C.c_int, P(vp)]
    L.gg_filter_cloud_pc2_out.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, P(C.c_double), P(C.c_float), C.c_double, vp, P(C.c_size_t)]
    L.gg_get_gridmap_message.argtypes = [vp, C.c_int, C.c_uint, P(GGGridMapHeader), vp, C.c_size_t, P(C.c_size_t)]
    L.gg_run_stage.argtypes = [vp, C.c_int, C.c_int, P(GGStageArgs)]
    L.gg_insert_cloud.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_size_t, P(C.c_float), vp, vp]
    L.gg_filter_cloud_layers.argtypes = [vp, C.c_int, vp, C.c_size_t, P(C.c_double), P(C.c_float), C.c_double, vp, P(C.c_size_t), vp, vp, P(vp)]
    L.gg_host_register.argtypes = [vp, vp, C.c_size_t]
    L.gg_host_unregister.argtypes = [vp, vp]
    L.gg_get_layer_image_u8.argtypes = [vp, C.c_int, C.c_int, vp, P(C.c_float), P(C.c_float)]
    L.gg_get_terrain_image.argtypes = [vp, C.c_int, vp]
    L.gg_filter_batch.argtypes = [vp, P(GGBatch), vp]
    L.gg_synchronize.argtypes = [vp]
    L.gg_device_error.argtypes = [vp, C.c_int]
    L.gg_batch_fence.argtypes = [vp, vp]
    L.gg_get_point_classes.argtypes = [vp, C.c_int, C.c_size_t, vp, vp]
    L.gg_get_kernel_times.argtypes = [vp, P(C.c_double), P(C.c_int64), C.c_int]
    L.gg_set_conventions.argtypes = [vp, P(GGConventions)]
    L.gg_get_conventions.argtypes = [vp, P(GGConventions)]
    L.gg_rotation_from_quaternion.argtypes = [C.c_int, P(C.c_double), P(C.c_double)]
    L.gg_transform_from_pose.argtypes = [C.c_int, P(C.c_double), P(C.c_double)]
    L.gg_filter_cloud_async.argtypes = [vp, C.c_int, vp, C.c_size_t, P(C.c_double), P(C.c_float), C.c_double, P(C.c_int)]
    L.gg_filter_cloud_wait.argtypes = [vp, C.c_int, vp, P(C.c_size_t), vp, vp]
    L.gg_collective_available.argtypes = []
    L.gg_comm_unique_id.argtypes = [vp]
    L.gg_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, P(vp)]
    L.gg_comm_init_rank_for.argtypes = [vp, vp, C.c_int, C.c_int, P(vp)]
    L.gg_comm_destroy.argtypes = [vp]
    L.gg_allgather_label_masks.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.gg_set_score_labels.argtypes = [vp, C.c_int, P(C.c_int32)]
    L.gg_set_slot_scoring.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, C.c_int]
    L.gg_get_slot_scores.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int, P(GGSlotScores)]
    L.gg_reset_slot_scores.argtypes = [vp, C.c_int, P(C.c_int32), C.c_int]
    L.gg_get_score_kernel_time.argtypes = [vp, P(C.c_double), P(C.c_int64), C.c_int]
    _lib = L
    return L
