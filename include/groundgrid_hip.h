/*
 * groundgrid_hip.h -- C ABI of libgroundgrid_hip.so: GroundGrid's per-cloud hot path on MI355X (gfx950).
 *
 * The reference has no FFI of its own for this path: it is the C++ class
 * groundgrid::GroundSegmentation in the separately linked library
 * groundgrid_groundsegmentation_lib (/root/reference/CMakeLists.txt:112-125), used by the nodelet
 * at src/GroundGridNodelet.cpp:95 (init), :301 (setConfig) and :196 (filter_cloud).  A drop-in
 * replacement of that library keeps the class (see groundgrid_amd/host/GroundSegmentation.hpp and
 * INTEGRATION.md) and forwards to the entry points below.  Each entry point cites the reference
 * interface it replaces.
 *
 * Conventions the reference never had: every function returns gg_status (0 = OK, negative =
 * error), nothing throws across the boundary, all state lives in an opaque gg_context.  Calls on
 * one context must be externally serialised (the reference's callbacks are serialised by the ROS
 * spinner, src/GroundGridNode.cpp:42); different contexts are independent.
 *
 * Plain pointers and sizes only -- no torch / HIP types in any signature (a HIP stream is passed
 * as void*).  The library fails loudly (GG_ERR_NO_DEVICE / GG_ERR_HIP): there is no CPU fallback.
 */
#ifndef GROUNDGRID_HIP_H
#define GROUNDGRID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_ABI_VERSION 6

typedef enum gg_status {
    GG_OK = 0,
    GG_ERR_INVALID = -1,   /* null pointer / bad argument                        */
    GG_ERR_GEOMETRY = -2,  /* grid_map size and GroundSegmentation::init cell count disagree, or a sensor constant of gg_geometry is negative or not finite */
    GG_ERR_NOMEM = -3,     /* device or host allocation failed                   */
    GG_ERR_HIP = -4,       /* a HIP runtime call or kernel failed (see gg_last_error) */
    GG_ERR_CAPACITY = -5,  /* cloud larger than max_points / slot out of range   */
    GG_ERR_NO_DEVICE = -6  /* no gfx950 device visible                           */
} gg_status;

/* velodyne_pointcloud::PointXYZIR, include/velodyne_pointcloud/point_types.h:27-33 (32 B, 16-B aligned) */
typedef struct gg_point32 {
    float x, y, z, pad0;
    float intensity;
    uint16_t ring;
    uint16_t pad1;
    uint32_t pad2[2];
} gg_point32;

/* Device-native packed record (what the host staging path uploads: everything the algorithm
 * reads of a point -- x, y, z, ring -- in one 16-B load). */
typedef struct gg_point16 {
    float x, y, z;
    uint16_t ring;
    uint16_t pad;
} gg_point16;

typedef enum gg_point_format { GG_POINT32 = 0, GG_POINT16 = 1 } gg_point_format;

/* groundgrid::GroundGridConfig, generated from cfg/GroundGrid.cfg:8-21 (int_t -> int, double_t -> double) */
typedef struct gg_config {
    int point_count_cell_variance_threshold;
    int max_ring;
    double groundpatch_detection_minimum_threshold;
    double distance_factor;
    double minimum_distance_factor;
    double miminum_point_height_threshold; /* sic */
    double minimum_point_height_obstacle_threshold;
    double outlier_tolerance;
    double ground_patch_detection_minimum_point_count_threshold;
    double patch_size_change_distance;
    double occupied_cells_decrease_factor;
    double occupied_cells_point_count_factor;
    double min_outlier_detection_ground_confidence;
    int thread_count; /* accepted and ignored: results are those of thread_count = 1 */
} gg_config;

/* Compile-time constants of the reference made run-time parameters:
 * GroundGrid::mDimension / mResolution (include/groundgrid/GroundGrid.h:70-71) and
 * GroundSegmentation::verticalPointAngDist / minDistSquared (include/groundgrid/GroundSegmentation.h:69-70).
 * Zero selects the reference value.  vertical_point_ang_dist (radians between two neighbouring beams: 32- and 128-beam sensors change
 * it) and min_dist_squared (m^2) must be finite and not negative: gg_create returns GG_ERR_GEOMETRY for a negative, infinite or NaN
 * value of either and creates no context. */
typedef struct gg_geometry {
    float length;                  /* 120.0f */
    float resolution;              /* .33f   */
    float vertical_point_ang_dist; /* (float)(0.00174532925*2) */
    float min_dist_squared;        /* 12.0f  */
} gg_geometry;

/* grid_map layer names used by the path (src/GroundGrid.cpp:55, src/GroundSegmentation.cpp:61-75) */
typedef enum gg_layer {
    GG_LAYER_POINTS = 0,
    GG_LAYER_GROUND = 1,
    GG_LAYER_GROUNDPATCH = 2,
    GG_LAYER_MINGROUNDHEIGHT = 3,
    GG_LAYER_MAXGROUNDHEIGHT = 4,
    GG_LAYER_GROUNDCANDIDATES = 5,
    GG_LAYER_PLANEDIST = 6,
    GG_LAYER_M2 = 7,
    GG_LAYER_MEANVARIANCE = 8,
    GG_LAYER_POINTSRAW = 9,
    GG_LAYER_VARIANCE = 10,
    GG_NUM_LAYERS = 11
} gg_layer;

/* per-input-point label: the intensity codes filter_cloud writes (src/GroundSegmentation.cpp:175,180,188);
 * 0 = the point is not in the returned cloud (outside the map, :230-231, or border, :167-168). */
enum { GG_LABEL_DROPPED = 0, GG_LABEL_GROUND = 49, GG_LABEL_NONGROUND = 99 };

/* per-input-point class decided by insert_cloud (src/GroundSegmentation.cpp:230-279) */
enum { GG_CLASS_OUTSIDE = 0, GG_CLASS_IGNORED = 1, GG_CLASS_OUTLIER = 2, GG_CLASS_KEPT = 3 };

/* gg_set_flags bits */
enum {
    GG_FLAG_MINIMAL_LAYERS = 1, /* the three layers nothing in the path reads (groundCandidates, planeDist, maxGroundHeight,
                                   src/GroundSegmentation.cpp:296,303,307) are not maintained per cloud; a reader of one of them
                                   (gg_get_layer, gg_get_layers, gg_get_layer_image_u8, gg_set_layer) has them computed first, from
                                   the tile-sorted records the slot's last cloud left on the device -- so every layer reads at all
                                   times as the reference's would.  Default: off for the calls that take or return host buffers (the
                                   binding publishes every layer), ON for gg_filter_batch -- device-resident clouds, nobody has asked
                                   for a layer -- unless GG_FLAG_EAGER_LAYERS is set */
    GG_FLAG_PROFILE = 2,        /* bracket every kernel with events on the launch stream (gg_get_kernel_times) */
    GG_FLAG_EAGER_LAYERS = 8,   /* gg_filter_batch maintains all nine per-call layers for every cloud as well (the behaviour up to ABI v5:
                                   k_reduce 1.27 instead of 1.11 ms per 1024 clouds) */
    GG_FLAG_CONCURRENT_HALVES = 4 /* a gg_filter_batch of at least 256 clouds runs as TWO independent launch sequences side by side: the
                                   clouds whose map slot is in the lower half of the context's slots on the caller's stream, the others
                                   on a stream of the library's own, and gg_reset_maps on a caller stream divides its fills the same way.
                                   A map slot is only ever touched from "its" stream, so the two sequences never wait for each other:
                                   they drift apart, kernels of different kinds overlap and fill each other's tails (+4 % clouds/s at
                                   1024 clouds per call).  An OUTPUT row follows a cloud's position in the batch, its half the cloud's slot: while
                                   every row keeps its half from batch to batch (or the output buffers are fresh) nothing joins; a batch that
                                   would write a row from the other stream than the batch before is ordered behind both first.  The price: the CALLER'S STREAM IS NOT ORDERED AFTER THE SECOND HALF.  Work the
                                   caller enqueues itself behind the call (copies of the outputs, its own kernels) must follow
                                   gg_batch_fence(ctx, stream) first; every gg_* entry point orders itself (getters, gg_synchronize,
                                   gg_allgather_label_masks, batches on other streams).  Ignored on the legacy default stream (its implicit synchronisation
                                   with every other stream makes two halves slower than one sequence) and while GG_FLAG_PROFILE is set: with two
                                   kernels sharing the device an event pair times half a machine, not a kernel.  Results identical. */
};

typedef struct gg_context gg_context;

/* ---- lifetime ------------------------------------------------------------------------------ */

void gg_default_config(gg_config *cfg);     /* cfg/GroundGrid.cfg defaults */
void gg_default_geometry(gg_geometry *g);   /* GroundGrid.h:70-71, GroundSegmentation.h:69-70 */

/* GroundSegmentation::init (src/GroundSegmentation.cpp:37-48) + the map geometry GroundGrid creates
 * (grid_map::setGeometry, src/GroundGrid.cpp:58), for n_slots independent map states ("streams")
 * that can be processed in one batched launch.  max_points = capacity per cloud. */
int gg_create(const gg_geometry *geom, int n_slots, size_t max_points, int device, gg_context **out);
void gg_destroy(gg_context *ctx);

/* GroundSegmentation::setConfig (src/GroundSegmentation.cpp:468-471).  Blocking, unlike the reference's struct copy: waits for the
 * batches in flight and rebuilds the per-cell threshold table of detect_ground_patches (O(cells) host work + one upload).  On failure
 * the context keeps its previous configuration entirely. */
int gg_set_config(gg_context *ctx, const gg_config *cfg);
int gg_get_config(const gg_context *ctx, gg_config *cfg);
/* Per-map configuration: every GroundSegmentation object of the reference has its own setConfig, so one context (one launch) may
 * mix them -- a 32-beam and a 64-beam vehicle in one fleet, or K candidate configurations of a parameter sweep as K slots.
 * slots[k] (or first_slot + k when slots == NULL) get their own configuration cfgs[k]; cfgs == NULL: those slots follow the
 * context's configuration (gg_set_config) again.  Blocks like gg_set_config: batches in flight finish with the old settings,
 * everything enqueued after the call returns uses the new ones.  GG_ERR_CAPACITY for a slot outside the context,
 * GG_ERR_INVALID for duplicates / n < 0 / null ctx; on any error no slot's configuration changes.  n == 0 is GG_OK.
 * A slot without its own configuration follows gg_set_config, later calls included; one with its own keeps it through
 * gg_set_config, gg_reset_map(s) and gg_move_map(s).  Every entry point that runs the path (or a stage of it) on a slot uses the
 * slot's configuration; gg_get_config still returns the context's.  thread_count is accepted and ignored. */
int gg_set_slot_configs(gg_context *ctx, int n, const int32_t *slots, int first_slot, const gg_config *cfgs);
/* the configuration slot `slot` runs with; *own = 1 if it has its own, 0 if it follows the context (own may be NULL) */
int gg_get_slot_config(const gg_context *ctx, int slot, gg_config *cfg, int *own);
#define GG_HAS_SLOT_CONFIG 1
int gg_set_flags(gg_context *ctx, unsigned flags);

/* Third-party conventions the reference inherits from the libraries it is built against (versions unpinned by the
 * reference: package.xml:29, CMakeLists.txt:41).  Each is one swappable function on the device and in the oracle;
 * tools/pin/ holds the probe that decides them on a real ROS box.
 *   eigen_reduction: order of Block<MatrixXf,5,5>::sum() / cwiseProduct().sum() (src/GroundSegmentation.cpp:359,374-375)
 *     GG_EIGEN_33       Eigen 3.3.x (Ubuntu 20.04 / ROS Noetic): DefaultTraversal + CompleteUnrolling, redux_novec_unroller
 *     GG_EIGEN_34_SSE   Eigen 3.4.x built for SSE2 (Packet4f): SliceVectorizedTraversal for the 5x5 blocks -- four row
 *                       lanes accumulated column by column, predux (a0+a2)+(a1+a3), then row 4 of every column
 *   The 3x3 blocks (:268, :457-458) take redux_novec_unroller under both versions. */
enum { GG_EIGEN_33 = 0, GG_EIGEN_34_SSE = 1 };
typedef struct gg_conventions {
    int eigen_reduction; /* GG_EIGEN_33 (default) */
    int reserved[7];     /* must be 0 */
} gg_conventions;
int gg_set_conventions(gg_context *ctx, const gg_conventions *conv);
int gg_get_conventions(const gg_context *ctx, gg_conventions *conv);

/* Quaternion (x, y, z, w) -> row-major 3x3 rotation the way the two candidates behind tf2::doTransform do it (host
 * arithmetic, no device involved):
 *   GG_ROT_TF2  tf2::Matrix3x3::setRotation (s = 2 / |q|^2; entries 1 - (yy + zz), xy - wz, ...): what
 *               doTransform(geometry_msgs::Point / Vector3, ...) and tf2::Transform use
 *   GG_ROT_KDL  KDL::Rotation::Quaternion (entries w2 + x2 - y2 - z2, 2xy - 2wz, ..., no normalisation): what
 *               tf2_geometry_msgs' doTransform(PointStamped) goes through (gmTransformToKDL) in ROS Melodic / Noetic --
 *               the overload the reference calls at src/GroundGrid.cpp:129 and src/GroundGridNodelet.cpp:146,176 */
enum { GG_ROT_TF2 = 0, GG_ROT_KDL = 1 };
int gg_rotation_from_quaternion(int convention, const double q_xyzw[4], double rot[9]);
/* {tx, ty, tz, qx, qy, qz, qw} -> 3x4 row-major (R | t) for gg_filter_cloud_tf / gg_batch.transforms, and the
 * {r20, r21, r22, tz} plane of gg_move_map */
int gg_transform_from_pose(int convention, const double pose7[7], double out12[12]);

int gg_get_size(const gg_context *ctx, int *rows, int *cols);          /* grid_map::GridMap::getSize */
int gg_get_geometry(const gg_context *ctx, double *resolution, double *length_x, double *length_y);
const char *gg_last_error(const gg_context *ctx);

/* ---- map state (what GroundGrid owns; the path borrows it by reference, :50) --------------- */

/* GroundGrid::initGroundGrid layer values (src/GroundGrid.cpp:71-75) + map position */
int gg_reset_map(gg_context *ctx, int slot, double pos_x, double pos_y, float odom_z);
/* The same for n_slots consecutive map states in one launch (position (pos_x, pos_y) and height odom_z for all).  With
 * persistent_only != 0 only the state that outlives a cloud is re-initialised -- ground := odom_z, groundpatch := 1e-7 -- which
 * is all a "cold" start needs: the nine per-call layers are rewritten by the next filter call anyway (:61-75).  Until then they read
 * as they stood (the three lazily kept ones as the map's last cloud left them), and the map position becomes (pos_x, pos_y) either way.
 * `stream`: NULL = the context's stream (like every other map mutation); a caller stream (or GG_STREAM_DEFAULT) enqueues the
 * fills there, ordered like a batch on that stream -- a server that re-initialises maps between batches on its own stream
 * then has no cross-stream hand-over in its loop.
 * Fresh maps (ABI v6, nothing to do for the caller): the (ground, groundpatch) layer of a re-initialised map is not written cell by cell
 * -- the library notes that it holds the reset's values, and a large gg_filter_batch of such maps sweeps them as they are (0.01 instead
 * of 0.35 ms per 1024 maps of 364 x 364); every other entry point that reads or edits the
 * layer (getters, setters, gg_move_map, the stage calls, single clouds, small or mixed batches) fills it first.  Every getter returns
 * the values above at all times.  Environment GG_FRESH_MAPS=0: write every cell, as before. */
int gg_reset_maps(gg_context *ctx, int first_slot, int n_slots, double pos_x, double pos_y, float odom_z, int persistent_only, void *stream);
/* map position after grid_map::move (src/GroundGrid.cpp:97); layers unchanged */
int gg_set_map_position(gg_context *ctx, int slot, double pos_x, double pos_y);
/* GroundGrid::update for an initialised map (src/GroundGrid.cpp:83-147): grid_map::GridMap::move to the odometry
 * position (whole cells; the map position is snapped), newly exposed cells get ground = -(z of the cell centre in
 * base_link) and groundpatch = 0 (:121-131), then convertToDefaultStartIndex (:143) -- on the device, so that the two
 * persistent layers never leave HBM between clouds.  ONLY those two scroll: the nine per-call layers are rewritten by the next filter call
 * (:61-75) and are left where they are -- a reader between the move and that call gets them as they stood before the move, where the
 * reference's grid_map::move would show them shifted, with NaN in the newly exposed cells (documented deviation; gg_move_maps alike).
 * base_plane = {r20, r21, r22, tz}: third row of the rotation and z of the translation of
 * lookupTransform("base_link", "map") (:103), i.e. z_base(p) = ((r20 * p.x + r21 * p.y) + r22 * p.z) + tz, evaluated in
 * this order in double (:129).  ABI v2: the caller hands over matrix entries, NOT a quaternion -- which rotation matrix
 * tf2::doTransform(PointStamped) builds from the quaternion (tf2::Matrix3x3::setRotation or KDL::Rotation::Quaternion)
 * is the binding's decision (gg_rotation_from_quaternion offers both).  shift (nullable) receives the index shift
 * (rows, cols). */
int gg_move_map(gg_context *ctx, int slot, double odom_x, double odom_y, const double base_plane[4], int shift[2]);
/* GroundGrid::update (src/GroundGrid.cpp:83-147) for n maps in one set of launches: map i = slots ? slots[i] : first_slot + i (distinct)
 * moves to (odom_xy[2i], odom_xy[2i+1]) with base_planes[4i..4i+3] exactly as gg_move_map(ctx, map i, ...) would -- the same shift,
 * position and cells, bit for bit.  A map whose shift is (0, 0) is not touched (it stays fresh, if it was).  A FRESH map (gg_reset_maps)
 * is scrolled as it is, without the fill gg_move_map puts first; the other fresh maps of the context stay fresh.  shifts (nullable)
 * receives [n][2] index shifts.  Enqueued on `stream` (NULL = the context's stream, GG_STREAM_DEFAULT or a caller stream: ordered like
 * gg_reset_maps there, and under GG_FLAG_CONCURRENT_HALVES the maps of the upper half of the slots scroll on the library's side stream);
 * returns without waiting, and the host arrays may be freed when it returns.  Errors change nothing: GG_ERR_INVALID (null ctx, null
 * odom_xy / base_planes with n > 0, repeated slots, n < 0), GG_ERR_CAPACITY (a slot outside the context), GG_ERR_NOMEM (the scratch
 * this entry point allocates at its first call -- at most 256 MB, one map layer per slot below that -- did not fit).  The first call
 * must not be captured into a graph.  n == 0 is GG_OK. */
int gg_move_maps(gg_context *ctx, int n, const int32_t *slots, int first_slot, const double *odom_xy, const double *base_planes, int32_t *shifts,
                 void *stream);
#define GG_HAS_MOVE_MAPS 1
int gg_get_map_position(const gg_context *ctx, int slot, double *pos_x, double *pos_y);
/* any of the 11 layers, column-major rows x cols float32 (Eigen::MatrixXf), host memory */
int gg_set_layer(gg_context *ctx, int slot, int layer, const float *src);
int gg_get_layer(gg_context *ctx, int slot, int layer, float *dst);
/* several layers in one go: dst[l] (nullable) receives layer l.  What the nodelet's publishers need after a cloud
 * (src/GroundGridNodelet.cpp:211-224 publishes every layer that has a subscriber): the extraction kernels and the downloads of
 * all requested layers are enqueued back to back and waited for once, instead of one synchronisation per layer. */
int gg_get_layers(gg_context *ctx, int slot, float *const dst[GG_NUM_LAYERS]);
/* The layers of n maps as dense planes in DEVICE memory, one launch, no synchronisation: what gg_get_layers returns for each of the
 * maps, bit for bit, where a consumer on the GPU (a planner, a model, a server that forwards terrain) can read it.
 * Map i = slots ? slots[i] : first_slot + i (distinct).  layer_mask has one bit per gg_layer, K = its popcount; the k-th requested
 * layer (in gg_layer order) of map i lands at d_dst + (i * K + k) * plane_stride.  plane_stride is in floats (>= rows * cols); the
 * elements between rows * cols and plane_stride are not written.  order: where cell (row, col) lies inside a plane. */
enum { GG_PLANES_COLMAJOR = 0,   /* cell (row, col) at row + col * rows: Eigen's order, what gg_get_layers returns */
       GG_PLANES_ROWMAJOR = 1 }; /* cell (row, col) at row * cols + col: image order, what the image getters use */
/* `stream` follows the gg_filter_batch convention (NULL = the context's stream, GG_STREAM_DEFAULT, or a caller stream).  The call
 * enqueues and returns: the host `slots` array may be freed on return, and work the caller enqueues on `stream` afterwards sees
 * the planes.  Ordering is the library's job, as for a batch: the export waits for every earlier map mutation and batch of the
 * context on other streams (both halves under GG_FLAG_CONCURRENT_HALVES), and every later entry point that writes one of the maps on
 * another stream waits for the export.
 * A FRESH map (gg_reset_maps, nothing since) exports ground = odom_z and groundpatch = 1e-7f without its layer being read or filled:
 * it, and every other fresh map of the context, stays fresh.  When layer_mask names maxGroundHeight, groundCandidates or planeDist,
 * the exported maps whose last cloud left them out (GG_FLAG_MINIMAL_LAYERS, the default of gg_filter_batch) get them computed first, in
 * one launch over exactly those maps on `stream`; a mask without the three launches nothing extra.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context), GG_ERR_INVALID (null ctx, n < 0,
 * repeated slots, layer_mask == 0 or with a bit at or above GG_NUM_LAYERS, unknown order, null d_dst, plane_stride < rows * cols -- the
 * last five only with n > 0).  n == 0 is GG_OK.  (A GG_ERR_HIP from the runtime in the middle of the call is not covered by that.)
 * The FIRST call of a context is slower and blocks: it builds the export table (6 bytes per cell) on the host, allocates it with the
 * call's parameter rings (GG_ERR_NOMEM when that does not fit) and uploads it with synchronous copies; later calls allocate nothing
 * and only enqueue.  Capturing the call into a caller's graph is neither supported nor tested: it waits on events that were recorded
 * outside the capture, and the first call allocates. */
int gg_export_layers(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned layer_mask, int order, float *d_dst,
                     size_t plane_stride, void *stream);
#define GG_HAS_EXPORT_LAYERS 1
/* The other direction: dense planes in DEVICE memory into the layers of n maps, one launch, no synchronisation.  Addressing mirrors
 * gg_export_layers exactly: map i = slots ? slots[i] : first_slot + i (distinct), K = popcount(layer_mask), the k-th named layer (in
 * gg_layer order) of map i is read from d_src + (i * K + k) * plane_stride, `order` is GG_PLANES_COLMAJOR or GG_PLANES_ROWMAJOR,
 * plane_stride is in floats (>= rows * cols) and the floats between rows * cols and plane_stride are never read.  d_src needs 4-byte
 * alignment only, and plane_stride may be odd.
 * After the call everything observable -- getters, exports, images, the gridmap message, gg_filter_*, gg_run_stage, gg_insert_cloud,
 * gg_move_map(s) -- is what it would be after gg_set_layer(ctx, slot_i, l, plane) for every named layer of every map, bit for bit
 * (NaN payloads and infinities included).  Layers that are not named keep their values; map positions, configurations, score counters
 * and conventions are untouched.  So gg_export_layers -> gg_import_layers -> continue is indistinguishable from never having left: a
 * checkpoint and roll-back, a map moved to another context or GPU, K candidates started from one warmed-up terrain.
 * `stream` follows the gg_filter_batch convention.  The call enqueues and returns: `slots` may be freed on return, d_src must stay valid
 * and unmodified until `stream` has passed the call.  The import is a map mutation and the library orders it like one: it waits for every
 * earlier mutation, batch and export of the context on other streams (both halves under GG_FLAG_CONCURRENT_HALVES), runs wholly on
 * `stream`, and every later entry point that reads or writes one of the maps on another stream waits for it.
 * A FRESH map (gg_reset_maps, nothing since) whose mask names ground and / or groundpatch becomes real by the import alone: the pair of
 * every cell is written, the component that is not named gets the reset's constant (odom_z / 1e-7f), nothing is filled first.  A fresh map
 * whose mask names neither, and every fresh map that is not listed, stays fresh.  The nine other layers share one set of liveness
 * marks per map: when the mask names any of them, all nine of a listed map become dense (imported ones take the plane, the others keep
 * their values and hold their per-call reset values wherever the last cloud wrote nothing).  Listed maps whose last cloud left
 * maxGroundHeight / groundCandidates / planeDist out (GG_FLAG_MINIMAL_LAYERS) get them computed first, in one launch over exactly those
 * maps on `stream` -- unless the mask names all three.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context), GG_ERR_INVALID (null ctx, n < 0,
 * repeated slots, layer_mask == 0 or with a bit at or above GG_NUM_LAYERS, unknown order, null d_src, plane_stride < rows * cols -- the
 * last five only with n > 0).  n == 0 is GG_OK.  (A GG_ERR_HIP from the runtime in the middle of the call is not covered by that.)
 * The call shares its table, parameter rings and events with gg_export_layers: the first of the two in a context allocates and
 * blocks, later calls only enqueue.  Capture into a caller's graph is not supported, as for the export. */
int gg_import_layers(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned layer_mask, int order, const float *d_src,
                     size_t plane_stride, void *stream);
#define GG_HAS_IMPORT_LAYERS 1
/* GroundSegmentation::expectedPoints (src/GroundSegmentation.cpp:40-46), host copy */
int gg_get_expected_points(const gg_context *ctx, float *dst);

/* ---- the hot path -------------------------------------------------------------------------- */

/* GroundSegmentation::filter_cloud (include/groundgrid/GroundSegmentation.h:54,
 * src/GroundSegmentation.cpp:50-197): host buffers in, host buffers out, synchronous.
 *   cloud, n    : input cloud already in the map frame (Nodelet.cpp:166-181)
 *   origin      : cloudOrigin x,y,z
 *   base_z      : mapToBase.transform.translation.z (the only field of the transform the path uses, :406-411)
 *   out_cloud   : capacity n (nullable); receives the returned cloud: kept, then ignored, then outliers
 *   out_n       : number of points in the returned cloud
 *   out_label   : per input point GG_LABEL_* (nullable)
 *   out_index   : per input point position in the returned cloud, -1 if dropped (nullable) */
int gg_filter_cloud(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const float origin[3],
                    double base_z, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label,
                    int32_t *out_index);

/* filter_cloud for a cloud that is still in the sensor frame: the per-point transform of points_callback
 * (src/GroundGridNodelet.cpp:148-184) is fused into the first kernel.  map_from_cloud = 3x4 row-major (R | t) of
 * lookupTransform("map", cloud frame).  The returned cloud is in the map frame, as in the reference. */
int gg_filter_cloud_tf(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double map_from_cloud[12],
                       const float origin[3], double base_z, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label,
                       int32_t *out_index);

/* Pipelined form of gg_filter_cloud / gg_filter_cloud_tf (map_from_cloud nullable): packs the cloud into one of
 * GG_ASYNC_DEPTH pinned staging buffers, enqueues upload + kernels + download and returns a ticket without waiting;
 * gg_filter_cloud_wait blocks until that cloud is done and hands out the results.  With two clouds in flight the
 * host-side packing and the H2D copy of cloud k+1 overlap the kernels of cloud k, and the result download / returned-
 * cloud assembly of cloud k overlaps the kernels of cloud k+1 (clouds of one slot still execute in call order: cloud k+1
 * reads the map state cloud k left).  `cloud` must stay valid until the matching wait when out_cloud is requested
 * there.  Tickets must be waited for in issue order; at most GG_ASYNC_DEPTH may be outstanding (GG_ERR_CAPACITY). */
#define GG_ASYNC_DEPTH 2
int gg_filter_cloud_async(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *map_from_cloud,
                          const float origin[3], double base_z, int *ticket);
int gg_filter_cloud_wait(gg_context *ctx, int ticket, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label,
                         int32_t *out_index);

/* filter_cloud AND the layers a publisher needs afterwards, as one call: what the nodelet does per cloud is filter_cloud followed
 * by reading every layer of the map (grid_map message + images, src/GroundGridNodelet.cpp:196-228).  layers[l] (nullable) receives
 * layer l, column-major rows x cols, like gg_get_layers -- but the eight layers that are final once the insertion has run
 * (minGroundHeight, maxGroundHeight, groundCandidates, planeDist, m2, meanVariance, pointsRaw, variance) are extracted and
 * downloaded on a side branch WHILE the patch stencil and the terrain sweep run, and ground / groundpatch / points follow the
 * per-point results while the host assembles the returned cloud.  map_from_cloud nullable (as gg_filter_cloud_async).
 * Destinations inside a range passed to gg_host_register are written by the device directly (no staging copy on the host): a host
 * whose map planes keep their addresses from cloud to cloud -- grid_map::GridMap does -- registers them once. */
int gg_filter_cloud_layers(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *map_from_cloud, const float origin[3],
                           double base_z, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label, int32_t *out_index,
                           float *const layers[GG_NUM_LAYERS]);
/* hipHostRegister / hipHostUnregister of a host range for a caller that has no HIP headers: downloads of this context whose
 * destination lies inside a registered range (gg_filter_cloud_layers) land there directly.  Unregister before freeing the memory;
 * gg_destroy unregisters what is left. */
int gg_host_register(gg_context *ctx, void *ptr, size_t bytes);
int gg_host_unregister(gg_context *ctx, void *ptr);

/* With GG_GRAPH=1 in the environment, one cloud per call (gg_filter_cloud*, gg_filter_batch with n_clouds == 1 on a stream other
 * than the legacy default one) replays a captured HIP graph from the third call of a kind on: the seven launches of the path reach
 * the device as one submission.  Off by default: measured, a replay is no faster than the eager launches. */

/* Batched, device-resident form of the same call: n_clouds independent (cloud, map-state) pairs in
 * one set of launches, slot first_slot + b (or slots[b]) for cloud b.  Pointers prefixed d_ are device memory.
 * Enqueues on `stream` (a hipStream_t passed as void*; NULL = the context's own stream, GG_STREAM_DEFAULT = the legacy
 * default ("null") stream, which as a hipStream_t is itself 0) and returns without waiting.
 * Ordering across streams is the library's job, not the caller's: a batch waits (hipStreamWaitEvent) for every earlier
 * map mutation of the context (gg_reset_map, gg_move_map, gg_set_layer, earlier batches on other streams), and every
 * later entry point that reads or writes map state on the context's own stream (gg_get_layer, gg_set_layer,
 * gg_move_map, gg_reset_map, the image / class getters, gg_filter_cloud*) waits for the batch.  The caller only has to
 * keep the buffers named in gg_batch alive and unmodified until the stream has passed the batch. */
typedef struct gg_batch {
    int n_clouds;
    int first_slot;
    int point_format;        /* gg_point_format */
    const void *d_points;    /* [n_clouds][cloud_stride] records of point_format */
    size_t cloud_stride;     /* in points; <= max_points */
    const int32_t *n_points; /* host [n_clouds] */
    const float *origins;    /* host [n_clouds][3] */
    const double *base_z;    /* host [n_clouds] */
    const double *transforms; /* host [n_clouds][12], nullable: map <- cloud frame as 3x4 row-major (R | t).  When given,
                                the points are still in the sensor frame and are transformed on the device exactly like
                                the nodelet does per point (tf2::doTransform in double, cast to float,
                                src/GroundGridNodelet.cpp:166-181); labels / returned clouds refer to map-frame points */
    uint8_t *d_labels;       /* [n_clouds][cloud_stride], nullable */
    int32_t *d_out_index;    /* [n_clouds][cloud_stride], nullable */
    gg_point32 *d_out_clouds; /* [n_clouds][cloud_stride], nullable; needs point_format == GG_POINT32 */
    int32_t *d_out_counts;   /* [n_clouds][4]: returned-cloud size, kept, ignored, outliers; nullable */
    uint8_t *d_label_masks;  /* [n_clouds][(cloud_stride + 3) / 4], nullable: the labels as a 2-bit mask, point p in bits
                                2*(p%4).. of byte p/4: 0 dropped, 1 ground (49), 2 non-ground (99) -- what a multi-GPU
                                caller all-gathers (a quarter of d_labels).  cloud_stride must be a multiple of 4; only the bytes
                                covering points < n_points (rounded up to a multiple of 64) are written */
    const int32_t *slots;    /* host [n_clouds], nullable (ABI v3): cloud b meets map slot slots[b] instead of first_slot + b
                                (first_slot is ignored then).  Entries must be distinct and inside the context: a server that
                                holds many streams' maps filters whichever of them received a cloud, in one set of launches */
    uint8_t *d_out_pc2;      /* [n_clouds][cloud_stride * GG_PC2_POINT_STEP], nullable (ABI v5): the returned cloud of cloud b --
                                kept, then ignored, then outliers, d_out_counts[b][0] records -- as sensor_msgs/PointCloud2 data in
                                the 18-byte layout of scripts/kitti_data_publisher.py:139-150 (x@0 y@4 z@8 intensity@12 float32,
                                ring@16 uint16; intensity = 49 / 99), written by the label kernel itself from either point format:
                                what a publisher sends (src/GroundGridNodelet.cpp:196-200) comes down as 18 B x returned points with
                                no host assembly.  (pcl::toROSMsg of PointXYZIR publishes the 32-byte struct as is: that layout is
                                d_out_clouds.) */
} gg_batch;
#define GG_PC2_POINT_STEP 18
#define GG_STREAM_DEFAULT ((void *)(intptr_t)-1)
int gg_filter_batch(gg_context *ctx, const gg_batch *batch, void *stream);
/* GG_FLAG_CONCURRENT_HALVES: orders `stream` (same convention) after both halves of every batch enqueued so far.  A no-op otherwise. */
int gg_batch_fence(gg_context *ctx, void *stream);
int gg_synchronize(gg_context *ctx);
/* The few places where a kernel waits for ANOTHER work-group (the sweep cut into parts, the tile scan cut into parts, the fused front
 * end) bound their waits; a wait that runs out leaves a code in a host-visible word instead of hanging.  Every gg_* call that
 * synchronises reports it ONCE as GG_ERR_HIP (text in gg_last_error) and clears it: the outputs of the batches enqueued since the
 * previous report are void and the map states they touched should be re-initialised (gg_reset_map); the context itself keeps
 * working.  A caller that synchronises its own stream instead of calling into the library asks here: returns the pending code
 * (0 = none, > 0 = a wait ran out) without synchronising; clear != 0 also clears it. */
int gg_device_error(gg_context *ctx, int clear);

/* ---- the score of a labelled cloud: per-map evaluator counters ------------------------------------------------------
 * The reference's evaluation node (scripts/eval_groundpoint_classifier.py:95-132) receives the RETURNED cloud, in which `ring`
 * carries the point's SemanticKITTI label (scripts/kitti_data_publisher.py:124-130) and `intensity` the prediction (49 ground /
 * 99 non-ground), and counts both predictions per label.  Here every map slot has such an evaluator on the device, fed by the
 * launches that filter the slot: K candidate configurations as K slots (gg_set_slot_configs) are scored without one label
 * leaving HBM.
 * What is counted: every input point that is in the returned cloud (label 49 or 99; dropped points never), in the bin of its
 * `ring` and under its label -- except a returned point whose map-frame z is NaN: pc2.read_points(..., skip_nans=True) (:99)
 * leaves out a point any of whose x, y, z is NaN, and a point inside the map has finite x and y, so z decides.  `total` of a
 * label (:118) is ground + non-ground; true / false positives and the summary figures (:153-195) are host arithmetic.
 * Every entry point that runs the label loop on a scoring slot accumulates: gg_filter_batch and gg_filter_cloud, _tf, _async /
 * _wait, _layers, _pc2, _pc2_out (`ring` from off_ring).  gg_insert_cloud and gg_run_stage do not label and do not score.  A
 * launch in which no slot scores runs the kernels it always ran.  Counters survive gg_reset_map(s), gg_move_map(s),
 * gg_set_config, gg_set_slot_configs and switching scoring off and on: an evaluator spans a whole sequence. */
#define GG_HAS_SCORES 1
#define GG_SCORE_MAX_LABELS 64
typedef struct gg_slot_scores {
    uint64_t clouds;                                /* filter calls scored (the evaluator's "Received N point clouds", :137) */
    uint64_t counts[GG_SCORE_MAX_LABELS + 1][2];    /* [bin][0] predicted non-ground, [bin][1] predicted ground */
} gg_slot_scores;
/* The label ids that get a bin of their own, in the caller's order: bin k counts ring == ids[k], bin n_ids every other id (the
 * reference raises KeyError for an id outside its yaml, :106: a documented deviation -- a caller that wants the reference's
 * behaviour treats a non-zero last bin as that error).  1 <= n_ids <= GG_SCORE_MAX_LABELS, each id in 0..65535, all distinct;
 * otherwise GG_ERR_INVALID and nothing changes.  The library holds no label table of its own.  Per context; blocks like
 * gg_set_config; zeroes the counters of every slot (the on / off state of the slots stays). */
int gg_set_score_labels(gg_context *ctx, int n_ids, const int32_t *ids);
/* Scoring on (enable != 0) or off for slots[k] (or first_slot + k when slots == NULL); off for every slot by default.  Slot
 * addressing and errors as gg_set_slot_configs: GG_ERR_CAPACITY for a slot outside the context, GG_ERR_INVALID for duplicates /
 * n < 0 / null ctx, and GG_ERR_INVALID while no label list is set; on any error nothing changes; n == 0 is GG_OK.  Blocks:
 * batches in flight finish under the old setting. */
int gg_set_slot_scoring(gg_context *ctx, int n, const int32_t *slots, int first_slot, int enable);
/* out[k] = the counters of slots[k] (or first_slot + k).  Orders itself after every batch enqueued so far (both halves under
 * GG_FLAG_CONCURRENT_HALVES) and synchronises, like the other getters -- but touches no map: fresh maps stay fresh.  Bins at and
 * above n_ids + 1 read 0, and so does every bin of a slot that never scored.  Same slot errors; GG_ERR_INVALID while no label
 * list is set or out == NULL with n > 0. */
int gg_get_slot_scores(gg_context *ctx, int n, const int32_t *slots, int first_slot, gg_slot_scores *out);
/* zero the counters of the named slots; their on / off state stays.  Blocks like gg_set_slot_scoring. */
int gg_reset_slot_scores(gg_context *ctx, int n, const int32_t *slots, int first_slot);

/* ---- the one collective of the path: the all-gather of the per-cloud label masks (BASELINE configs[2]) ----
 * The reference has no distributed code; clouds shard as independent (cloud, map) pairs and the only exchange is that every
 * rank ends up with every cloud's labels.  These entry points let a C / C++ host run that configuration without Python:
 * they bind RCCL (librccl.so, the ROCm build of the NCCL API) at run time with dlopen, so the library has no link-time
 * dependency on it and a single-GPU user never loads it.
 *
 *   gg_comm_unique_id       rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by whatever means
 *                           the host has (MPI, a socket, torch.distributed ...)
 *   gg_comm_init_rank       every rank: ncclCommInitRank on the CURRENT HIP device -> an opaque communicator (ncclComm_t)
 *   gg_comm_init_rank_for   the same on the device of `ctx` (selected first): what a caller that holds a context wants -- with one
 *                           rank, or a transport that never touched HIP, nothing else has selected a device yet (ABI v4)
 *   gg_allgather_label_masks  ncclAllGather(d_send, d_recv, bytes_per_rank, ncclUint8) on `stream` (same convention as
 *                           gg_filter_batch: NULL = the context's stream, GG_STREAM_DEFAULT = the legacy default stream); d_send =
 *                           this rank's gg_batch.d_label_masks (or d_labels), d_recv = [world][bytes_per_rank].  The call is
 *                           ordered after the context's last batch (event wait when the streams differ) and returns without
 *                           waiting; `comm` may be any ncclComm_t, also one the host created itself.  The library remembers the
 *                           send buffer: a later gg_filter_batch on ANOTHER stream whose d_label_masks / d_labels overlap it is
 *                           ordered after the gather (event wait) -- batches that write other buffers (double buffering) are not
 *   gg_comm_destroy
 * GG_ERR_NO_DEVICE when librccl.so cannot be loaded, GG_ERR_HIP for RCCL errors (text in gg_last_error). */
int gg_collective_available(void);
int gg_comm_unique_id(uint8_t id_out[128]);
int gg_comm_init_rank(const uint8_t id[128], int n_ranks, int rank, void **comm_out);
int gg_comm_init_rank_for(gg_context *ctx, const uint8_t id[128], int n_ranks, int rank, void **comm_out);
int gg_comm_destroy(void *comm);
int gg_allgather_label_masks(gg_context *ctx, void *comm, const uint8_t *d_send, uint8_t *d_recv, size_t bytes_per_rank, void *stream);

/* ---- wire formats around the path (src/GroundGridNodelet.cpp:120, :211-291) -------------------------------------- */

/* filter_cloud straight from a sensor_msgs/PointCloud2 payload (e.g. the KITTI player's 18-byte records,
 * scripts/kitti_data_publisher.py:139-150: x@0 y@4 z@8 intensity@12 ring@16): one host pass packs the fields the path
 * reads, instead of pcl::fromROSMsg into 32-byte points first (Nodelet.cpp:120).  map_from_cloud (nullable) as in
 * gg_filter_cloud_tf.  Results per input point; the caller owns the payload and can assemble whatever message it needs. */
int gg_filter_cloud_pc2(gg_context *ctx, int slot, const uint8_t *data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                        size_t off_z, size_t off_ring, const double *map_from_cloud, const float origin[3], double base_z,
                        uint8_t *out_label, int32_t *out_index, size_t *out_n);
/* PointCloud2 payload in, PointCloud2 payload out: the same call with the RETURNED CLOUD written as 18-byte records (x, y, z,
 * intensity = 49 / 99, ring; the layout above, gg_batch.d_out_pc2) by the label kernel -- order kept, ignored, outliers as in
 * src/GroundSegmentation.cpp:150-189 -- so that the download is 18 B per returned point and the host assembles nothing.  out_data
 * needs room for n * GG_PC2_POINT_STEP bytes; *out_n = points of the returned cloud (= width x height of the message, row_step =
 * 18 * width).  The input layout is free (point_step / offsets) as for gg_filter_cloud_pc2. */
int gg_filter_cloud_pc2_out(gg_context *ctx, int slot, const uint8_t *data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                            size_t off_z, size_t off_ring, const double *map_from_cloud, const float origin[3], double base_z,
                            uint8_t *out_data, size_t *out_n);

/* The map as the serialised grid_map_msgs/GridMap the nodelet publishes per cloud (src/GroundGridNodelet.cpp:211-214:
 * grid_map::GridMapRosConverter::toMessage, info.header.stamp := the cloud's stamp): ROS 1 wire format, little endian --
 *   info   { header {seq, stamp, frame_id}, resolution, length_x, length_y, pose {position (map x, map y, 0), orientation (0,0,0,1)} }
 *   layers[], basic_layers[]    names in the order the reference adds them (src/GroundGrid.cpp:55, src/GroundSegmentation.cpp:61-75)
 *   data[]  one std_msgs/Float32MultiArray per layer: dim[0] {"column_index", cols, rows*cols}, dim[1] {"row_index", rows, rows},
 *           data_offset 0, data = the layer column-major (Eigen's storage, copied as is)
 *   outer_start_index = inner_start_index = 0 (GroundGrid::update ends with convertToDefaultStartIndex, src/GroundGrid.cpp:143)
 * restated from grid_map_ros 1.6.x (GridMapRosConverter::toMessage, GridMapMsgHelpers: not under /root/reference, unpinned).
 * layer_mask: bit per gg_layer (0 = all eleven).  The layer planes are extracted by one kernel, come down in one copy and are
 * placed straight into the message.  dst == NULL or capacity too small: only *size is set (GG_ERR_CAPACITY in the second case). */
typedef struct gg_gridmap_header {
    uint32_t seq;
    uint32_t stamp_sec, stamp_nsec;
    const char *frame_id;   /* NULL = "map" (src/GroundGrid.cpp:57) */
    unsigned basic_layers;  /* bit per gg_layer; the reference declares none */
} gg_gridmap_header;
int gg_get_gridmap_message(gg_context *ctx, int slot, unsigned layer_mask, const gg_gridmap_header *header, uint8_t *dst, size_t capacity, size_t *size);

/* grid_map::GridMapCvConverter::toImage<unsigned char, 1> of one layer (Nodelet.cpp:239): rows x cols row-major bytes,
 * the layer normalised between the min and max of its finite cells (returned in lower / upper), non-finite cells 0.
 * cv::applyColorMap (:240) is left to the host. */
int gg_get_layer_image_u8(gg_context *ctx, int slot, int layer, uint8_t *dst, float *lower, float *upper);
/* the 32FC3 terrain image (Nodelet.cpp:247-268): rows x cols x 3 floats (ground, 3x3 pointsRaw sum >= 27, pointsRaw) */
int gg_get_terrain_image(gg_context *ctx, int slot, float *dst);

/* Both images of MANY maps in DEVICE memory, in one call and without a synchronisation: what the two getters above return per map and
 * layer, where a consumer on the GPU (a model that takes the terrain tensor, a server that forwards BEV images) reads it.
 * Map i = slots ? slots[i] : first_slot + i (distinct, inside the context), as for gg_export_layers.
 *   u8 images   layer_mask has one bit per gg_layer (0: none), K = its popcount.  The image of the k-th named layer (in gg_layer order)
 *               of map i lies at d_images + (i * K + k) * image_stride: rows x cols row-major bytes, byte for byte what
 *               gg_get_layer_image_u8 writes.  image_stride is in bytes (>= rows * cols); the bytes between rows * cols and the stride
 *               are never written; neither d_images nor image_stride needs any alignment.  d_bounds (nullable): [n][K][2] floats, the
 *               lower and upper the getter returns -- (+inf, -inf) for a plane without a finite cell.
 *   terrain     d_terrain (nullable): the 32FC3 image of map i at d_terrain + i * terrain_stride, terrain_stride in floats
 *               (>= 3 * rows * cols; the floats behind the image are never written).  terrain_layout: GG_TERRAIN_HWC = rows x cols x 3
 *               interleaved -- what gg_get_terrain_image returns, bit for bit, a cv::Mat of type 32FC3 -- or GG_TERRAIN_CHW = three
 *               row-major rows x cols planes (ground, flag, pointsRaw), what a model takes.
 * `stream` follows the gg_filter_batch convention; the call enqueues and returns, `slots` may be freed on return, and work enqueued on
 * `stream` afterwards sees the images.  The library orders the call exactly like gg_export_layers (both halves under
 * GG_FLAG_CONCURRENT_HALVES included), and later writers of these maps on other streams wait for it.
 * A FRESH map (gg_reset_maps, nothing since) is neither read nor filled: its ground plane is the constant odom_z and its groundpatch
 * plane 1e-7f -- their u8 images are what the getter gives for a constant plane --, its terrain channel 0 is odom_z, and it and every other
 * fresh map stay fresh.  When layer_mask names maxGroundHeight, groundCandidates or planeDist, the listed maps whose last cloud left
 * them out get them computed first, in one launch over exactly those maps on `stream`; the terrain image needs none of the three.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context), GG_ERR_INVALID (null ctx, null x,
 * n < 0, repeated slots; and with n > 0: a mask bit at or above GG_NUM_LAYERS, layer_mask != 0 with null d_images, layer_mask == 0 with
 * null d_terrain -- nothing asked for --, image_stride < rows * cols, terrain_stride < 3 * rows * cols, an unknown terrain_layout).
 * n == 0 is GG_OK.  The call shares its table, parameter rings and events with gg_export_layers / gg_import_layers: the first of the
 * three in a context allocates and blocks, later calls only enqueue.  Capture into a caller's graph is not supported. */
enum { GG_TERRAIN_HWC = 0, GG_TERRAIN_CHW = 1 };
typedef struct gg_image_export {
    int n;                 /* maps */
    int first_slot;        /* map i = first_slot + i when slots == NULL */
    const int32_t *slots;  /* host [n], nullable */
    unsigned layer_mask;   /* the u8 images: bit per gg_layer, may be 0 */
    uint8_t *d_images;     /* [n][K] images, image_stride bytes apart; needed when layer_mask != 0 */
    size_t image_stride;   /* bytes, >= rows * cols */
    float *d_bounds;       /* [n][K][2] lower, upper; nullable */
    float *d_terrain;      /* [n] terrain images, terrain_stride floats apart; nullable */
    size_t terrain_stride; /* floats, >= 3 * rows * cols */
    int terrain_layout;    /* GG_TERRAIN_HWC / GG_TERRAIN_CHW */
} gg_image_export;
int gg_export_images(gg_context *ctx, const gg_image_export *x, void *stream);
#define GG_HAS_EXPORT_IMAGES 1

/* The point side of a batch in DEVICE memory: the ground and the non-ground points of MANY labelled clouds as two dense clouds per input
 * cloud, every point with its height above the estimated terrain and its index in the input -- what `points[labels == 99]` gives per
 * cloud, without the launch and the device -> host synchronisation per cloud that a data-dependent size costs: the counts stay on the
 * device.  Cloud i meets map slots ? slots[i] : first_slot + i (distinct, inside the context).
 *   selection   point p < n_points[i] of cloud i goes into `ground` when its label is 49 (GG_LABEL_GROUND) and into `nonground` when it
 *               is 99 (GG_LABEL_NONGROUND); any other label byte selects nothing.  The labels come as bytes (d_labels) or as the 2-bit masks
 *               of gg_batch.d_label_masks (d_label_masks; codes 1 and 2) -- exactly one of the two.
 *   order       ascending p, the cloud's own order: what cloud[labels == 99] gives, NOT the kept / ignored / outlier order of the
 *               returned cloud (gg_batch.d_out_clouds).
 *   addressing  row i of every output starts at i * cloud_stride elements.  d_counts[i] = {points in ground, points in nonground}.
 *               Never written: the elements at and beyond a row's count, and the rows of a set none of whose three pointers is given.
 *               Each of the three pointers of a set may be null on its own.
 *   records     x, y, z are the input's -- with `transforms`, the map-frame point the path computes from it (tf2::doTransform in double,
 *               cast to float, as for gg_batch.transforms): the bits of gg_batch.d_out_clouds / d_out_pc2.  ring is copied (gg_point16.ring,
 *               or offset 20 of a 32-byte point), pad is 0.
 *   height      one float subtraction, z_map - g: g is the `ground` layer of the cloud's map AS IT STANDS WHEN THE CALL RUNS, at the cell of
 *               the map-frame (x, y) under the map's current position (the path's own inside test and index arithmetic, :222-231).  Right
 *               behind gg_filter_batch on the same stream g is the value the label loop compared the point with
 *               (src/GroundSegmentation.cpp:162).  A selected point outside the map -- possible only when the caller's labels do not belong
 *               to these points and maps -- gets the quiet NaN 0x7FC00000 and reads nothing: the call is memory-safe for any label bytes.
 * The call is stateless with respect to the last cloud: it reads the caller's buffers, the maps' `ground` layer and their positions, and no
 * record a batch left behind -- any time, any maps, any labels.  A FRESH map (gg_reset_maps, nothing since) is neither read nor filled: its g
 * is the constant odom_z, and it and every other fresh map stay fresh.  None of the nine per-call layers is read (the three lazily kept ones
 * stay pending), and no layer, position, configuration, score or liveness flag changes.
 * `stream` follows the gg_filter_batch convention; the call enqueues and returns, the host arrays may be freed on return, and work enqueued
 * on `stream` afterwards sees the outputs.  The library orders the call exactly like gg_export_layers: it waits for every earlier map
 * mutation, batch, export and import of the context (both halves under GG_FLAG_CONCURRENT_HALVES), and later writers of these maps on
 * other streams wait for it.  The caller's buffers must stay valid and unmodified until `stream` has passed the call.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context, cloud_stride or an n_points[i] above
 * max_points), GG_ERR_INVALID (null ctx, null x, n < 0, repeated slots; and with n > 0: null d_points, n_points or d_counts, an unknown
 * point_format, both or neither of d_labels / d_label_masks, masks with a cloud_stride that is not a multiple of 4, n_points[i] < 0 or
 * > cloud_stride).  n == 0 is GG_OK.  The first call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.
 * Capture into a caller's graph is not supported. */
typedef struct gg_split_set {      /* one selected set of every cloud; each pointer nullable */
    gg_point16 *d_points;          /* [n][cloud_stride] x, y, z in the MAP frame, ring, pad = 0 */
    float      *d_height;          /* [n][cloud_stride] z - ground(cell of the point) */
    int32_t    *d_source;          /* [n][cloud_stride] index of the point in its input cloud */
} gg_split_set;
typedef struct gg_cloud_split {
    int n;                         /* clouds */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const uint8_t *d_labels;       /* [n][cloud_stride] GG_LABEL_*  -- exactly one of these two */
    const uint8_t *d_label_masks;  /* [n][(cloud_stride + 3) / 4] 2-bit masks, as gg_batch.d_label_masks */
    gg_split_set ground;           /* label 49 */
    gg_split_set nonground;        /* label 99 */
    int32_t *d_counts;             /* [n][2]: points in ground, in nonground; required */
} gg_cloud_split;
int gg_split_clouds(gg_context *ctx, const gg_cloud_split *x, void *stream);
#define GG_HAS_SPLIT_CLOUDS 1

/* The OBSTACLE GRID of a batch in DEVICE memory: per cell of every map how many non-ground points of the map's cloud fell there and how far
 * the highest and the lowest of them stand above the estimated terrain -- and the same three planes for the ground points (the height
 * residual of the terrain estimate) -- what a planner or a BEV model takes from a ground segmenter.  The reference keeps only the count
 * (the `points` layer, src/GroundSegmentation.cpp:147,176) and never a height.  One call for many maps, one pass over the points; cloud i
 * meets map slots ? slots[i] : first_slot + i (distinct, inside the context).
 *   selection   as gg_split_clouds: point p < n_points[i] belongs to the ground set when its label is 49 (mask code 1) and to the non-ground
 *               set when it is 99 (mask code 2); any other label byte selects nothing.  Labels as bytes or as 2-bit masks, exactly one.
 *   cell        of the map-frame (x, y) -- with `transforms`, of the point the path computes (tf2::doTransform in double, cast to float) --
 *               under the map's current position: the path's own inside test and index arithmetic (:222-231).  A selected point outside
 *               the map contributes to nothing: the call is memory-safe for any label bytes and any coordinates.
 *   height      h = z_map - g, one float subtraction; g is the `ground` layer of the cloud's map AS IT STANDS WHEN THE CALL RUNS.
 *   count       GG_RASTER_*_COUNT: the number of points of the set in the cell, as a float (exact: counts stay far below 2^24); an empty
 *               cell holds 0.0f.  Right behind gg_filter_batch on the same stream the non-ground count is the `points` layer bit for bit.
 *   max, min    GG_RASTER_*_MAX_HEIGHT / _MIN_HEIGHT: over the set's points in the cell whose h is not NaN, by IEEE totalOrder on the
 *               non-NaN values (-0.0 < +0.0, +-inf take part).  A cell without such a point holds the quiet NaN 0x7FC00000.  A point whose
 *               h is NaN (a NaN z, a NaN ground, inf - inf) is still counted.
 *   addressing  with K = popcount(channel_mask), the k-th named channel (in GG_RASTER_* order) of cloud i is the plane of rows * cols floats
 *               at d_dst + (i * K + k) * plane_stride, cell (row, col) where `order` (GG_PLANES_*) puts it.  EVERY cell of every named plane
 *               of every listed cloud is written, those of an empty cloud (n_points[i] == 0) included; the floats between rows * cols and
 *               plane_stride never are.  d_dst needs 4-byte alignment only.  While the call runs the planes hold intermediate words.
 *   determinism the result does not depend on the order in which points arrive: counts are integer atomic adds, heights integer atomic
 *               max / min on an order-preserving key of the float's bits; no float is ever added.  Bit-identical from run to run.
 * The call is stateless with respect to the last cloud, exactly as gg_split_clouds: it reads the caller's buffers, the maps' `ground` layer
 * and their positions, and no record a batch left behind.  A FRESH map is neither read nor filled: its g is the constant odom_z, and it and
 * every other fresh map stay fresh.  None of the nine per-call layers is read (the three lazily kept ones stay pending), and no layer,
 * position, configuration, score or liveness flag changes.
 * `stream` and ordering are those of gg_split_clouds: the call enqueues and returns, the host arrays may be freed on return, it waits for
 * every earlier map mutation, batch, export and import of the context (both halves under GG_FLAG_CONCURRENT_HALVES), and later writers of
 * these maps on other streams wait for it.  The caller's buffers must stay valid and unmodified until `stream` has passed the call.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context, cloud_stride or an n_points[i] above
 * max_points), GG_ERR_INVALID (null ctx, null x, n < 0, repeated slots; and with n > 0: null d_points, n_points or d_dst, an unknown
 * point_format or order, both or neither of d_labels / d_label_masks, masks with a cloud_stride that is not a multiple of 4, n_points[i] < 0
 * or > cloud_stride, channel_mask == 0 or with a bit at or above GG_NUM_RASTER_CHANNELS, plane_stride < rows * cols).  n == 0 is GG_OK.  The
 * first call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
enum { GG_RASTER_NONGROUND_COUNT = 0, GG_RASTER_NONGROUND_MAX_HEIGHT = 1, GG_RASTER_NONGROUND_MIN_HEIGHT = 2,
       GG_RASTER_GROUND_COUNT = 3,    GG_RASTER_GROUND_MAX_HEIGHT = 4,    GG_RASTER_GROUND_MIN_HEIGHT = 5,
       GG_NUM_RASTER_CHANNELS = 6 };
typedef struct gg_cloud_raster {
    int n;                         /* clouds */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const uint8_t *d_labels;       /* [n][cloud_stride] GG_LABEL_*  -- exactly one of these two */
    const uint8_t *d_label_masks;  /* [n][(cloud_stride + 3) / 4] 2-bit masks, as gg_batch.d_label_masks */
    unsigned channel_mask;         /* bit per GG_RASTER_*; K = its popcount, != 0 */
    int order;                     /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR */
    float *d_dst;                  /* [n][K] planes, plane_stride floats apart */
    size_t plane_stride;           /* floats, >= rows * cols */
} gg_cloud_raster;
int gg_rasterize_clouds(gg_context *ctx, const gg_cloud_raster *x, void *stream);
#define GG_HAS_RASTERIZE_CLOUDS 1

/* The SHAPE of the terrain of n maps as dense planes in DEVICE memory, one launch, no synchronisation: per cell how steep the ground is and
 * in which direction, how large the step to a neighbour is and how far the estimate can be trusted there -- what a planner otherwise builds
 * from gg_export_layers(ground, groundpatch) and two dozen passes of shifted slices.
 * Addressing, `order`, `plane_stride`, `stream`, slot lists and the ordering guarantees are exactly those of gg_export_layers: map i =
 * slots ? slots[i] : first_slot + i (distinct), K = popcount(channel_mask), the k-th named channel (in GG_SLOPE_* order) of map i goes to
 * d_dst + (i * K + k) * plane_stride; d_dst needs 4-byte alignment only and plane_stride (floats, >= rows * cols) may be odd; the floats
 * between rows * cols and plane_stride are not written; order is GG_PLANES_COLMAJOR or GG_PLANES_ROWMAJOR.
 * The call is stateless: it reads the `ground` and `groundpatch` layer of the listed maps as they stand, reads none of the nine per-call
 * layers, launches nothing for the three lazily kept ones (they stay pending), and changes no map, no flag, no score, no position.
 * DEFINITION.  With g = ground, w = groundpatch, res = the `float` resolution of gg_geometry, and for cell (r, c):
 *   r_lo = max(r-1, 0), r_hi = min(r+1, rows-1), c_lo = max(c-1, 0), c_hi = min(c+1, cols-1).
 *   All arithmetic is float32, with no contraction, IEEE division and square root, and denormals kept.
 *   GRAD_X          gx = (g(r_lo,c) - g(r_hi,c)) / ((float)(r_hi - r_lo) * res).  This is dz/dx in the map frame, because rows grow towards
 *                   -x.  It is one-sided on the border rows.
 *   GRAD_Y          gy = (g(r,c_lo) - g(r,c_hi)) / ((float)(c_hi - c_lo) * res)   (columns grow towards -y)
 *   TANGENT         sqrtf(gx*gx + gy*gy), the tangent of the slope angle.
 *   NORMAL_Z        1.0f / sqrtf((gx*gx + gy*gy) + 1.0f), the z component of the unit normal, equal to the cosine of the slope angle.
 *   STEP            m = 0.0f, then over the cells (r', c') of {r_lo..r_hi} x {c_lo..c_hi} other than (r, c), in any order:
 *                   m = fmaxf(m, fabsf(g(r',c') - g(r,c))).  A NaN difference is skipped, so the result is never NaN and its sign bit is
 *                   clear.
 *   MIN_CONFIDENCE  fminf of w over all cells of {r_lo..r_hi} x {c_lo..c_hi}, centre included, starting from w(r,c).  NaNs are skipped
 *                   unless all are NaN.
 * The first four channels are NaN where their stencil holds a NaN, or where inf - inf arises.  Which NaN is not specified.  Everything else
 * is specified to the bit.
 * A FRESH map (gg_reset_maps, nothing since) gets +0, +0, +0, 1.0f, +0, 1e-7f.  Its layer is not read or filled, and it and every other
 * fresh map stays fresh.
 * Argument errors write nothing and change nothing: GG_ERR_CAPACITY (a slot outside the context), GG_ERR_INVALID (null ctx, n < 0, repeated
 * slots, channel_mask == 0 or with a bit at or above GG_NUM_SLOPE_CHANNELS, unknown order, null d_dst, plane_stride < rows * cols -- the last
 * five only with n > 0).  n == 0 is GG_OK.  The call shares its table, parameter rings and events with gg_export_layers: the first of them
 * in a context allocates and blocks, later calls only enqueue.  Capture into a caller's graph is not supported, as for the export. */
enum { GG_SLOPE_GRAD_X = 0, GG_SLOPE_GRAD_Y = 1, GG_SLOPE_TANGENT = 2, GG_SLOPE_NORMAL_Z = 3,
       GG_SLOPE_STEP = 4, GG_SLOPE_MIN_CONFIDENCE = 5, GG_NUM_SLOPE_CHANNELS = 6 };
int gg_export_slopes(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned channel_mask, int order,
                     float *d_dst, size_t plane_stride, void *stream);
#define GG_HAS_EXPORT_SLOPES 1

/* The OBSTACLE CLUSTERS of a batch in DEVICE memory: the connected components of the occupied cells of every cloud's obstacle grid -- the
 * objects -- as a plane of cluster ids, a table of the clusters and a cluster id per point: the step that follows a ground segmenter, which
 * a caller otherwise composes from gg_rasterize_clouds, a download, a connected-components pass per map on the host and an upload.  One call
 * for many maps; cloud i meets map slots ? slots[i] : first_slot + i (distinct, inside the context).  The ten leading members are those of
 * gg_cloud_raster, with the same meaning and the same checks.
 *   participation  point p < n_points[i] of cloud i participates when (1) its label is 99 (mask code 2; any other byte selects nothing),
 *               (2) it lies inside its map by the path's own inside test and index arithmetic (:222-231) under the map's current position --
 *               with `transforms`, tested on the map-frame point the path computes -- and (3) its height h = z_map - g satisfies
 *               !(h < min_height) && !(h > max_height).
 *   height      h is one float subtraction against the `ground` layer of the cloud's map AS IT STANDS WHEN THE CALL RUNS.  A NaN h
 *               participates; min_height = -INFINITY and max_height = +INFINITY admit everything.  A FRESH map's g is its constant odom_z.
 *   occupied    a cell is occupied when at least min_points points participate in it.
 *   cluster     a connected component of occupied cells.  Under connectivity 4 the neighbours of (r, c) are (r +- 1, c) and (r, c +- 1);
 *               under connectivity 8 the four diagonals as well.  Nothing wraps at the border: (r, cols - 1) and (r + 1, 0) are not
 *               neighbours, although their row-major indices are consecutive.
 *   numbering   the clusters of a map are numbered 0 .. K-1 in ascending order of their smallest linear cell index, the index being that of
 *               `order`: r * cols + c for GG_PLANES_ROWMAJOR, r + c * rows for GG_PLANES_COLMAJOR.  With row-major order the plane is what
 *               scipy.ndimage.label(occupied, structure)[0] - 1 gives.  The partition does not depend on `order`; the numbering does.
 *   d_cell_cluster  cloud i's plane of rows * cols int32 at d_cell_cluster + i * plane_stride, cell (row, col) where `order` puts it.  EVERY
 *               cell of every listed plane is written: -1 where the cell is not occupied, else its cluster id.  The words between
 *               rows * cols and plane_stride never are.  4-byte alignment.  While the call runs the planes hold intermediate words.
 *   d_n_clusters[i]  K_i, the true count, also when it exceeds max_clusters.
 *   d_point_cluster[i][p]  for p < n_points[i] the id of the point's cell when the point participates and the cell is occupied, else -1.
 *               Elements at and beyond n_points[i] are never written.
 *   d_clusters[i][k]  written for k < min(K_i, max_clusters), every field; records at and beyond that never are.  cells: the cluster's
 *               occupied cells; points: the participating points in them; the four bounds: over its cells; first_cell: its smallest linear
 *               cell index, in `order`; height_max: the largest h of the cluster's participating points, by IEEE totalOrder on the non-NaN
 *               values (-0.0 < +0.0, +-inf take part), and the quiet NaN 0x7FC00000 when none of them has a non-NaN h.
 *   determinism only integer atomics (add, min, max) are used -- heights go through an order-preserving key of the float's bits -- and no
 *               float is ever added: the outputs are bit-identical from run to run and independent of scheduling.
 * The call is stateless exactly as gg_rasterize_clouds is: it reads the caller's buffers, the maps' `ground` layer and their positions, and
 * no record a batch left behind.  A FRESH map is neither read nor filled, and it and every other fresh map stay fresh.  None of the nine
 * per-call layers is read (the three lazily kept ones stay pending), and no layer, position, configuration, score or liveness flag changes.
 * `stream` and ordering are those of gg_rasterize_clouds: the call enqueues and returns, the host arrays may be freed on return, it waits for
 * every earlier map mutation, batch, export and import of the context (both halves under GG_FLAG_CONCURRENT_HALVES), and later writers of
 * these maps on other streams wait for it.  The caller's buffers must stay valid and unmodified until `stream` has passed the call.
 * Argument errors write nothing and change nothing: every error of gg_rasterize_clouds for the ten shared members, and GG_ERR_INVALID for
 * null ctx (before the device is touched), null x, n < 0; and with n > 0: null d_cell_cluster or d_n_clusters, min_points < 1, a
 * connectivity that is not 4 or 8, an unknown order, plane_stride < rows * cols, max_clusters < 0, d_clusters given with max_clusters == 0,
 * a NaN min_height or max_height.  n == 0 is GG_OK before anything else is looked at.  The first call of a context may allocate
 * (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
typedef struct gg_cluster {        /* 32 bytes */
    int32_t cells;                 /* occupied cells of the cluster */
    int32_t points;                /* participating points in those cells */
    int32_t row_min, row_max, col_min, col_max;
    float   height_max;            /* largest height of its participating points; 0x7FC00000: none that is not NaN */
    int32_t first_cell;            /* smallest linear cell index of the cluster, in `order` */
} gg_cluster;
typedef struct gg_cloud_clusters {
    int n;                         /* clouds */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const uint8_t *d_labels;       /* [n][cloud_stride] GG_LABEL_*  -- exactly one of these two */
    const uint8_t *d_label_masks;  /* [n][(cloud_stride + 3) / 4] 2-bit masks, as gg_batch.d_label_masks */
    int min_points;                /* >= 1: participating points that make a cell occupied */
    float min_height, max_height;  /* the height band (not NaN; -INFINITY / +INFINITY: open) */
    int connectivity;              /* 4 or 8 */
    int order;                     /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR */
    int32_t *d_cell_cluster;       /* [n] planes of rows * cols int32, plane_stride apart; required */
    size_t plane_stride;           /* int32 words, >= rows * cols */
    int32_t *d_point_cluster;      /* [n][cloud_stride], nullable */
    int32_t *d_n_clusters;         /* [n], required */
    gg_cluster *d_clusters;        /* [n][max_clusters], nullable */
    int max_clusters;              /* >= 0; must be > 0 when d_clusters is given */
} gg_cloud_clusters;
int gg_cluster_clouds(gg_context *ctx, const gg_cloud_clusters *x, void *stream);
#define GG_HAS_CLUSTER_CLOUDS 1

/* The CLEARANCE of a batch in DEVICE memory: per cell of every map how far the nearest occupied cell is and which one it is -- the exact
 * Euclidean distance transform of the obstacle grid with its feature transform, what costmap inflation, clearance checks along a path and
 * "nearest object" look-ups start from, and what a caller otherwise composes from gg_cluster_clouds, a download,
 * scipy.ndimage.distance_transform_edt per map on the host and an upload.  One call for many maps, in exactly one of two modes:
 *   cloud mode  d_points != NULL and d_seeds == NULL.  The ten leading members are those of gg_cloud_raster, with the same meaning and the
 *               same checks; cloud i meets map slots ? slots[i] : first_slot + i.  A cell is occupied exactly where gg_cluster_clouds,
 *               given the same ten members, min_points, min_height and max_height, writes d_cell_cluster >= 0: participation (label 99 /
 *               mask code 2, the path's own inside test, !(h < min_height) && !(h > max_height), a NaN h participates, a FRESH map's ground
 *               is its constant odom_z) and the threshold min_points are its, computed by the same launches.
 *   seed mode   d_seeds != NULL.  Map i's occupancy is the plane of rows * cols int32 at d_seeds + i * seed_stride, cell (row, col) where
 *               `order` puts it; a cell is occupied when its word is >= 0: a d_cell_cluster plane of gg_cluster_clouds plugs in as it is,
 *               and so does any plane the caller thresholds into {-1, 0}.  d_points, n_points, transforms, d_labels, d_label_masks and slots
 *               must be NULL; point_format, cloud_stride, first_slot, min_points, min_height and max_height are ignored.  No map is read;
 *               n may not exceed the context's n_slots.  d_seeds may not overlap an output.
 * For cell (r, c), over the occupied cells (r', c') of the same map, nothing wrapping at the border:
 *   d_dist2     the minimum of (r - r')^2 + (c - c')^2: an exact integer, 0 on an occupied cell.
 *   d_nearest   the linear index, in `order` (r' * cols + c' for GG_PLANES_ROWMAJOR, r' + c' * rows for GG_PLANES_COLMAJOR), of the occupied
 *               cell that attains the minimum; among several the one with the smallest r', then the smallest c'.  The tie rule does not
 *               depend on `order`.
 *   d_distance  sqrtf((float)dist2) * res, res the `float` resolution of gg_geometry: IEEE square root, one multiplication, no contraction.
 *   max_cells   R > 0: a cell whose dist2 > R * R is reported as having no obstacle; every other value is that of R = 0 (unbounded).
 *   no obstacle (an empty map, or beyond R): d_dist2 = GG_CLEARANCE_NONE, d_nearest = -1, d_distance = +inf (0x7F800000).
 *   d_n_occupied[i]  the number of occupied cells of map i, whatever max_cells is.
 *   addressing  map i's plane of rows * cols words at <output> + i * plane_stride, cell (row, col) where `order` puts it.  EVERY cell of
 *               every given plane of every listed map is written, an empty cloud's (n_points[i] == 0) included; the words between
 *               rows * cols and plane_stride never are, and an output whose pointer is NULL is not touched.  4-byte alignment.  d_dist2 is
 *               required: it is the working memory of the call and holds intermediate words while it runs.
 *   determinism integer arithmetic and one integer atomic add only: bit-identical from run to run and independent of scheduling.
 * Cloud mode is stateless exactly as gg_rasterize_clouds is: it reads the caller's buffers, the maps' `ground` layer and their positions.
 * A FRESH map is neither read nor filled, and it and every other fresh map stay fresh; the lazily kept layers stay pending; no layer,
 * position, configuration, score or liveness flag changes.  `stream` and ordering are those of gg_rasterize_clouds: the call enqueues and
 * returns, the host arrays may be freed on return, it waits for every earlier map mutation, batch, export and import of the context, and
 * later writers of these maps on other streams wait for it.  Seed mode takes an entry of the same ring and orders itself the same way, but
 * reads no map.  The caller's buffers must stay valid and unmodified until `stream` has passed the call.
 * Argument errors write nothing and change nothing: in cloud mode every error of gg_rasterize_clouds for the ten shared members; and
 * GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with n > 0: both or neither of d_points and d_seeds, a
 * cloud member (n_points, transforms, d_labels, d_label_masks, slots) set in seed mode, seed_stride < rows * cols in seed mode, null
 * d_dist2, plane_stride < rows * cols, an unknown order, max_cells < 0, and in cloud mode min_points < 1 or a NaN min_height or max_height;
 * GG_ERR_CAPACITY for n > n_slots in seed mode.  n == 0 is GG_OK before anything else is looked at.  The first call of a context may
 * allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
#define GG_CLEARANCE_NONE 0x7FFFFFFF
typedef struct gg_cloud_clearance {
    int n;                         /* clouds (cloud mode) / maps (seed mode) */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points; NULL: seed mode */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const uint8_t *d_labels;       /* [n][cloud_stride] GG_LABEL_*  -- exactly one of these two (cloud mode) */
    const uint8_t *d_label_masks;  /* [n][(cloud_stride + 3) / 4] 2-bit masks, as gg_batch.d_label_masks */
    int min_points;                /* >= 1: participating points that make a cell occupied, as gg_cloud_clusters */
    float min_height, max_height;  /* the height band (not NaN; -INFINITY / +INFINITY: open), as gg_cloud_clusters */
    const int32_t *d_seeds;        /* [n] planes of rows * cols int32, seed_stride apart: occupied where >= 0; NULL: cloud mode */
    size_t seed_stride;            /* int32 words, >= rows * cols */
    int max_cells;                 /* 0: unbounded; R > 0: no obstacle is reported beyond R cells */
    int order;                     /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR */
    int32_t *d_dist2;              /* [n] planes of rows * cols int32, plane_stride apart; required: the call's working memory */
    size_t plane_stride;           /* 32-bit words, >= rows * cols, of all three kinds of plane */
    int32_t *d_nearest;            /* [n] planes, nullable */
    float   *d_distance;           /* [n] planes, nullable */
    int32_t *d_n_occupied;         /* [n], nullable */
} gg_cloud_clearance;
int gg_clearance_clouds(gg_context *ctx, const gg_cloud_clearance *x, void *stream);
#define GG_HAS_CLEARANCE_CLOUDS 1

/* The VISIBILITY of a batch in DEVICE memory: per cell of every map whether the sensor saw it free, saw an obstacle in it, or never saw it
 * -- the third state a clearance field lacks (gg_clearance_clouds gives a cell behind a wall as much clearance as one a hundred beams
 * crossed), what costmap_2d's obstacle layer clears by ray tracing, what exploration takes its frontiers from, and what a caller otherwise
 * composes from a download of the clouds and a ray walk per point on the host.  One call for many clouds.  The ten leading members are
 * those of gg_cloud_raster, with the same meaning and the same checks; cloud i meets map slots ? slots[i] : first_slot + i.
 *   occupied    exactly where gg_cluster_clouds, given the same ten members, min_points, min_height and max_height, writes
 *               d_cell_cluster >= 0: participation (label 99 / mask code 2, the path's own inside test, !(h < min_height) &&
 *               !(h > max_height), a NaN h participates, a FRESH map's ground is its constant odom_z) and the threshold min_points are
 *               its, computed by the same launches, as gg_clearance_clouds does in cloud mode.
 *   hit         a cell in which at least one point p < n_points[i] lands whose label is 49 or 99 (mask code 1 or 2); the cell is that of
 *               the path's inside test, on the map-frame point when `transforms` is given.  A point outside the map and any other label
 *               byte contribute nothing, neither a hit nor a ray: RETURNS BEYOND THE MAP'S EDGE CLEAR NOTHING INSIDE IT.
 *   sensor cell (r0, c0), the cell of ((double)origins[i][0], (double)origins[i][1]) by the same inside test and index arithmetic under
 *               the map's current position.  When the origin lies outside the map or is not finite, cloud i casts no ray; its hits and
 *               its occupancy still count.
 *   ray         of a hit cell (r1, c1): with dr = r1 - r0, dc = c1 - c0 and n = max(|dr|, |dc|), for k = 0 .. n-1 -- and only k < R when
 *               max_cells = R > 0 -- the cell
 *                   (r0 + sgn(dr) * ((2 k |dr| + n) / (2 n)), c0 + sgn(dc) * ((2 k |dc| + n) / (2 n)))     (integer division)
 *               is CROSSED: k d / n rounded to the nearest integer, halves away from zero.  The sensor cell is crossed, the end cell is
 *               not; consecutive cells are 8-neighbours; the eight octants mirror each other exactly; n = 0 crosses nothing.  One ray per
 *               distinct hit cell: the ray depends on (sensor cell, end cell) alone.  The implementation relies on 2 n n + n < 2^24 (every
 *               term is then exact in a float as well) and on one bit per cell fitting a work-group's local memory: rows * cols <=
 *               1 308 672 (a side of 1143); a context with a larger map gets GG_ERR_GEOMETRY from this call.
 *   state       GG_CELL_OCCUPIED where occupied; else GG_CELL_FREE where hit or crossed; else GG_CELL_UNKNOWN.  A ray is not stopped by
 *               an occupied cell on its way: the return behind it was measured.
 *   d_counts[i] the number of cells of map i in each state, in the order free, unknown, occupied; they sum to rows * cols.
 *   values      FREE < 0 <= UNKNOWN < OCCUPIED: a state plane is a seed plane of gg_clearance_clouds as it stands (cells >= 0, "occupied or
 *               never observed", are its seeds), which gives the conservative clearance.
 *   addressing  cloud i's plane of rows * cols int32 at d_state + i * plane_stride, cell (row, col) where `order` puts it.  EVERY cell of
 *               every listed plane is written, an empty cloud's included (all GG_CELL_UNKNOWN, counts {0, rows * cols, 0}); the words
 *               between rows * cols and plane_stride never are, and d_counts is not touched when NULL.  4-byte alignment.  d_state is the
 *               working memory of the call and holds intermediate words while it runs.
 *   determinism integer arithmetic and integer atomics (add, and) only: bit-identical from run to run and independent of scheduling.
 * The call is stateless exactly as gg_rasterize_clouds is: it reads the caller's buffers, the maps' `ground` layer and their positions, and
 * no record a batch left behind.  A FRESH map is neither read nor filled, and it and every other fresh map stay fresh.  None of the nine
 * per-call layers is read (the three lazily kept ones stay pending), and no layer, position, configuration, score or liveness flag changes.
 * `stream` and ordering are those of gg_rasterize_clouds: the call enqueues and returns, the host arrays (origins included) may be freed on
 * return, it waits for every earlier map mutation, batch, export and import of the context (both halves under GG_FLAG_CONCURRENT_HALVES),
 * and later writers of these maps on other streams wait for it; it takes an entry of the same ring of parameter entries.  The caller's
 * buffers must stay valid and unmodified until `stream` has passed the call.
 * Argument errors write nothing and change nothing: every error of gg_rasterize_clouds for the ten shared members, and GG_ERR_INVALID for
 * null ctx (before the device is touched), null x, n < 0; and with n > 0: null origins or d_state, plane_stride < rows * cols, an unknown
 * order, max_cells < 0, min_points < 1, a NaN min_height or max_height; GG_ERR_GEOMETRY for a map of more cells than stated above.
 * n == 0 is GG_OK before anything else is looked at.  The first call of a context may allocate (GG_ERR_NOMEM) and block; later calls only
 * enqueue.  Capture into a caller's graph is not supported. */
enum { GG_CELL_FREE = -1, GG_CELL_UNKNOWN = 0, GG_CELL_OCCUPIED = 1 };
typedef struct gg_cloud_visibility {
    int n;                         /* clouds */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const uint8_t *d_labels;       /* [n][cloud_stride] GG_LABEL_*  -- exactly one of these two */
    const uint8_t *d_label_masks;  /* [n][(cloud_stride + 3) / 4] 2-bit masks, as gg_batch.d_label_masks */
    int min_points;                /* >= 1: participating points that make a cell occupied, as gg_cloud_clusters */
    float min_height, max_height;  /* the height band (not NaN; -INFINITY / +INFINITY: open), as gg_cloud_clusters */
    const float *origins;          /* host [n][3], required: the sensor in the MAP frame, as gg_batch.origins; only x, y are used */
    int max_cells;                 /* 0: unbounded; R > 0: a ray clears at most its first R cells */
    int order;                     /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR */
    int32_t *d_state;              /* [n] planes of rows * cols int32, plane_stride apart; required: the call's working memory */
    size_t plane_stride;           /* int32 words, >= rows * cols */
    int32_t *d_counts;             /* [n][3]: free, unknown, occupied cells of map i; nullable */
} gg_cloud_visibility;
int gg_visibility_clouds(gg_context *ctx, const gg_cloud_visibility *x, void *stream);
#define GG_HAS_VISIBILITY_CLOUDS 1

/* The occupancy grid that PERSISTS ACROSS SCANS, in DEVICE memory: gg_visibility_clouds describes one scan -- most far cells of a rotating
 * LiDAR are GG_CELL_UNKNOWN in any single one, and an obstacle that drops out of one scan is gone from that scan's plane -- while a costmap
 * accumulates.  gg_fuse_states carries one int32 of EVIDENCE per cell of many maps from scan to scan: it scrolls the previous evidence by
 * the index shift gg_move_maps returned, lets it decay towards 0, adds this scan's observation, clamps, and writes the new evidence, the
 * three-valued state it gives, the exploration frontier and the counts, in one launch.  What a caller otherwise composes per frame from a
 * shifted copy into a zeroed buffer, a where, a clamp, two thresholds and an eight-neighbour pooling pass -- with the sign of the shift to
 * get right.  Map i of the call is row i of every buffer and of `shifts`; with (s0, s1) = (shifts[2 i], shifts[2 i + 1]) (both 0 when
 * `shifts` is NULL), for cell (r, c), all in 32-bit integers:
 *   prior        (r', c') = (r + s0, c + s1), nothing wraps.  P = 0 when r' lies outside [0, rows) or c' outside [0, cols) -- so for every
 *                cell when |s0| >= rows or |s1| >= cols -- or when d_evidence_in is NULL; otherwise P = clamp(in[r', c'], e_min, e_max), `in`
 *                being map i's plane of d_evidence_in.  This is the rule of gg_move_maps for the map's own layers, new(r, c) = exposed ?
 *                fill : old(r + s0, c + s1): a cell that gg_move_maps fills as newly exposed starts here without evidence.  THE SHIFT IS THE
 *                ONE gg_move_maps RETURNED FOR THE MOVE BETWEEN THE TWO OBSERVATIONS: between the scan d_evidence_in was fused from and
 *                the scan of d_state; of several moves in between, the sum of their shifts.
 *   decay        D = P > 0 ? max(P - decay, 0) : min(P + decay, 0).
 *   observation  with s = map i's d_state[r, c]:  E = clamp(D + (s > 0 ? hit : s < 0 ? -miss : 0), e_min, e_max).  A d_state plane of
 *                gg_visibility_clouds fits as it stands (GG_CELL_OCCUPIED > 0, GG_CELL_FREE < 0, GG_CELL_UNKNOWN = 0 "not observed"); any
 *                other positive or negative word counts by its sign alone.  d_evidence_out[r, c] = E.
 *   fused state  F = GG_CELL_OCCUPIED if E >= occ_threshold, else GG_CELL_FREE if E <= free_threshold, else GG_CELL_UNKNOWN.
 *                d_fused[r, c] = F.
 *   frontier     d_frontier[r, c] = 0 where F == GG_CELL_FREE and at least one of the up to eight neighbours (r + a, c + b), a, b in
 *                {-1, 0, 1}, inside the map has F == GG_CELL_UNKNOWN; -1 everywhere else.  Cells beyond the border are no neighbours.
 *   d_counts[i]  the number of cells of map i with F free, unknown, occupied (they sum to rows * cols), then the number of zeros of its
 *                frontier plane.  The frontier is counted whether or not d_frontier is given.
 *   limits       0 <= hit, miss, decay <= 2^30 - 1;  -(2^30 - 1) <= e_min <= 0 <= e_max <= 2^30 - 1;  e_min <= free_threshold <= -1;
 *                1 <= occ_threshold <= e_max: every sum above then stays inside an int32.  The C ABI has no defaults.
 *   values       a fused plane is a seed plane of gg_clearance_clouds as it stands (cells >= 0: occupied or never observed: the
 *                conservative clearance), and so is a frontier plane (the distance to the nearest frontier cell, and which cell it is).
 *   addressing   map i's plane of rows * cols int32 at d_state + i * state_stride, and at d_evidence_in / d_evidence_out / d_fused /
 *                d_frontier + i * plane_stride; cell (row, col) where `order` puts it, the same order for every plane of the call.  EVERY
 *                cell of every given output plane of every map is written; the words between rows * cols and a stride never are, and a
 *                NULL output is not touched.  4-byte alignment.
 *   no overlap   no output may share a byte with an input or with another output: the prior is read at shifted cells and the frontier from
 *                neighbours, so NO UPDATE IN PLACE IS DEFINED -- the caller alternates between two evidence buffers.  The call compares
 *                the address ranges, each from a buffer's first word to the last cell of its last plane (planes of two buffers interleaved
 *                in each other's slack count as overlapping), and answers GG_ERR_INVALID.  d_state and d_evidence_in may overlap each other.
 *   determinism  integer arithmetic and integer atomic adds only: bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_clearance_clouds in seed mode: NO MAP IS READ OR CHANGED -- no layer, position, freshness, configuration, score
 * or liveness flag, and the lazily kept layers stay pending; the evidence lives in the caller's buffers, not in the context.  n <= n_slots
 * (GG_ERR_CAPACITY): the call takes an entry of the same ring of parameter entries (the shifts travel in it) and orders itself on `stream`
 * exactly as that call does; it enqueues and returns, and `shifts` may be freed on return.  The caller's device buffers must stay valid and
 * unmodified until `stream` has passed the call.
 * ORDER OF THE MANY-MAP CALLS ACROSS STREAMS, for the caller's buffers too: a call that takes a `stream` (gg_filter_batch, gg_reset_maps,
 * gg_move_maps, gg_export_layers, gg_import_layers and every call declared below gg_export_layers, this one and the five plane calls after it
 * included) starts its device work only when the device work of every such call the host issued earlier on the same context has finished,
 * on whichever stream either one runs (the context's own, GG_STREAM_DEFAULT or a caller's).  So a plane this call reads may be one that an
 * earlier call on another stream writes (d_state straight from gg_visibility_clouds, d_evidence_in from the last gg_fuse_states), and a
 * buffer this call writes may be one that an earlier call on another stream still reads (the evidence buffer of two calls ago), with no event
 * or synchronisation of the caller's between the two.  What the caller itself enqueues -- a fill, a copy, a kernel of its own -- is ordered by
 * its stream alone: work on `stream` in front of the call is seen by it, work behind it sees the call, and nothing else is promised.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_state or d_evidence_out, state_stride or plane_stride < rows * cols, an unknown order, a parameter outside the limits above,
 * overlapping buffers; GG_ERR_CAPACITY for n > n_slots.  n == 0 is GG_OK before anything else is looked at.  The first many-map call of a
 * context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
typedef struct gg_state_fusion {
    int n;                          /* maps */
    const int32_t *d_state;         /* [n] observation planes, state_stride apart: > 0 occupied, < 0 free, 0 not observed
                                       (a d_state plane of gg_visibility_clouds as it stands); required */
    size_t state_stride;            /* int32 words, >= rows * cols */
    const int32_t *d_evidence_in;   /* [n] evidence planes of the previous call, plane_stride apart; NULL: every prior is 0 */
    const int32_t *shifts;          /* host [n][2] index shifts (rows, cols) as gg_move_maps returns them; NULL: all (0, 0) */
    int hit, miss, decay;           /* >= 0 */
    int e_min, e_max;               /* e_min <= 0 <= e_max */
    int free_threshold, occ_threshold; /* free_threshold <= -1, occ_threshold >= 1 */
    int order;                      /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    int32_t *d_evidence_out;        /* [n] planes, plane_stride apart; required */
    size_t plane_stride;            /* int32 words, >= rows * cols: evidence in/out, fused, frontier */
    int32_t *d_fused;               /* [n] planes GG_CELL_*; nullable */
    int32_t *d_frontier;            /* [n] planes: 0 on a frontier cell, -1 elsewhere; nullable */
    int32_t *d_counts;              /* [n][4]: free, unknown, occupied, frontier cells; nullable */
} gg_state_fusion;
int gg_fuse_states(gg_context *ctx, const gg_state_fusion *x, void *stream);
#define GG_HAS_FUSE_STATES 1

/* The NAVIGATION FUNCTION of many maps, in DEVICE memory: gg_fuse_states ends with a persistent three-valued grid and an exploration frontier
 * per map, and gg_clearance_clouds with a frontier plane as seeds gives the distance to the nearest frontier THROUGH walls.  gg_route_planes
 * gives the distance AROUND them: per cell the exact cost D of the cheapest admissible 4- or 8-connected path to the nearest goal cell over a
 * caller-given cost plane, the next cell on that path, three counts per map and, from one start cell per map, the cell list of the path.  What
 * a caller otherwise gets per map and per frame from a download of three planes, a graph, Dijkstra on the host and an upload.  The goal set (a
 * d_frontier plane) and the blocked set (a d_fused plane) are read as they stand.  Map i of the call is row i of every buffer and of `starts`.
 * Everything is 32-bit integer; nothing wraps at the border; all of the following is per map:
 *   blocked      cell q is BLOCKED where map i's d_blocked word is >= 0 (no cell when d_blocked is NULL).
 *   weight       w(q) = min(max(word of d_cost, 1), cost_max); 1 everywhere when d_cost is NULL.
 *   goal         a cell whose d_goals word is >= 0 and that is not blocked.  A blocked goal is no goal.
 *   step         from q = (r, c) to p = (r + a, c + b): the straight steps (a, b) in {(-1,0), (0,-1), (0,+1), (+1,0)} always, the four
 *                diagonals with connectivity 8.  ADMISSIBLE when p lies inside the map and neither p nor q is blocked, and for a diagonal
 *                when (r + a, c) and (r, c + b) are both inside and unblocked as well: no corner cutting.  It costs s * w(p): s = `straight`
 *                or `diagonal`, w of the cell ENTERED.
 *   D            0 on a goal; elsewhere the minimum, over all finite chains of admissible steps from q to a goal, of the sum of the step
 *                costs; GG_ROUTE_NONE where there is no such chain (a blocked cell, a pocket, a map without goals).  Equivalently D is the
 *                unique solution of D(q) = min over admissible p of D(p) + s * w(p) with D = 0 on the goals, which makes it independent of
 *                how it is computed.  d_dist[q] = D(q).
 *   limits       1 <= straight, diagonal <= 65535; 1 <= cost_max; max(straight, diagonal) * cost_max * rows * cols <= 2^31 - 2, `diagonal`
 *                counted with connectivity 8 only.  Every true D then fits an int32, every word the call stores while it works is
 *                <= 2^31 - 1 and one step costs <= 2^31 - 2, so the UNSIGNED sum of a stored word and a step cannot wrap: the kernel relies
 *                on that.  The C ABI has no defaults.
 *   max_cost     R > 0: a cell with D > R gets d_dist = GG_ROUTE_NONE and d_next = -1 and is not counted as reached; every other word is
 *                that of R = 0 (a prefix of a cheapest path is cheaper, so the bounded field is consistent).  0: unbounded.
 *   d_next       a goal's own linear index; -1 on an unreached cell; otherwise the linear index, in `order`, of the FIRST p in the direction
 *                order (-1,0), (0,-1), (0,+1), (+1,0), (-1,-1), (-1,+1), (+1,-1), (+1,+1) whose step is admissible and attains D(q) =
 *                D(p) + s * w(p).  Directions are in (row, col) terms: the tie rule does not depend on `order`.  Following d_next lowers D
 *                by at least 1 per step: every chain ends on a goal and has no cycle.
 *   d_counts[i]  the number of goals, of reached cells (goals included; under max_cost), and of unblocked cells.
 *   paths        with `starts`, map i's path is starts[i], next(starts[i]), ... up to and including the goal.  d_path_len[i] is the number
 *                of cells of the whole path, also when that exceeds max_path; d_paths[i][k] is written for k < min(len, max_path) and the
 *                other words of the row never are.  d_path_len[i] = 0 and the row is untouched when starts[i] is -1 or an unreached cell
 *                (blocked cells and cells beyond max_cost included).  A start on a goal gives len 1.  starts[i] is a linear index in
 *                `order`.  d_next need not be given for the paths.
 *   values       a d_fused or d_frontier plane of gg_fuse_states, a d_state plane of gg_visibility_clouds and a d_cell_cluster plane of
 *                gg_cluster_clouds fit d_blocked and d_goals as they stand.
 *   addressing   map i's plane of rows * cols int32 at d_blocked + i * blocked_stride, d_cost + i * cost_stride, d_goals + i * goal_stride
 *                and d_dist / d_next + i * plane_stride; cell (row, col) where `order` puts it, the same order for every plane of the call.
 *                EVERY cell of every given output plane of every map is written; the words between rows * cols and a stride never are,
 *                and a NULL output is not touched.  d_dist is the call's working memory.  4-byte alignment.
 *   no overlap   no output may share a byte with an input or with another output; the call compares the address ranges as gg_fuse_states
 *                does and answers GG_ERR_INVALID.  The inputs may overlap each other.
 *   determinism  integer arithmetic only; D is a unique fixed point and d_next and the paths are functions of D: bit-identical from run to
 *                run and independent of scheduling.
 * The contract is that of gg_clearance_clouds in seed mode and of gg_fuse_states: NO MAP IS READ OR CHANGED -- no layer, position, freshness,
 * configuration, score or liveness flag, and the lazily kept layers stay pending.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry
 * of the same ring of parameter entries (the starts travel in it) and orders itself on `stream` as those calls do; it enqueues and returns
 * with no synchronisation, and `starts` may be freed on return.  The caller's device buffers must stay valid and unmodified until `stream`
 * has passed the call.  One work-group computes one map's D, so many maps fill the device and a single map runs on one compute unit.
 * Across streams the call is ordered, for the caller's buffers too, as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_goals or d_dist, a stride < rows * cols for a given plane, an unknown order, connectivity not 4 or 8, a parameter outside
 * the limits above, max_cost < 0, `starts` given without d_paths, d_path_len or max_path >= 1, a starts[i] < -1 or >= rows * cols,
 * overlapping buffers; GG_ERR_CAPACITY for n > n_slots; GG_ERR_GEOMETRY for a map of more than 4096 tiles of 64 x 64 cells.  n == 0 is
 * GG_OK before anything else is looked at.  The first many-map call of a context may allocate (GG_ERR_NOMEM) and block; later calls only
 * enqueue.  Capture into a caller's graph is not supported. */
#define GG_ROUTE_NONE 0x7FFFFFFF
typedef struct gg_plane_routes {
    int n;                        /* maps */
    const int32_t *d_blocked;     /* [n] planes, blocked_stride apart: a cell is BLOCKED where the word is >= 0 (a d_fused plane of
                                     gg_fuse_states, a d_state plane, a d_cell_cluster plane as they stand); NULL: nothing is blocked */
    size_t blocked_stride;
    const int32_t *d_cost;        /* [n] planes, cost_stride apart: w = min(max(word, 1), cost_max); NULL: w = 1 everywhere */
    size_t cost_stride;
    const int32_t *d_goals;       /* [n] planes, goal_stride apart: a GOAL where the word is >= 0 and the cell is not blocked
                                     (a d_frontier plane of gg_fuse_states as it stands); required */
    size_t goal_stride;
    int connectivity;             /* 4 or 8 */
    int straight, diagonal;       /* step weights, e.g. 5 and 7; diagonal is ignored with connectivity 4 */
    int cost_max;                 /* >= 1 */
    int max_cost;                 /* 0: unbounded; R > 0: a cell whose D > R is reported as unreached */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    int32_t *d_dist;              /* [n] planes, plane_stride apart; required: the call's working memory */
    size_t plane_stride;          /* d_dist and d_next */
    int32_t *d_next;              /* [n] planes; nullable */
    int32_t *d_counts;            /* [n][3]: goals, reached cells (goals included), unblocked cells; nullable */
    const int32_t *starts;        /* host [n]: linear index in `order` of map i's start cell, or -1; nullable */
    int32_t *d_paths;             /* [n][max_path]; required when starts is given */
    int max_path;                 /* >= 1 when starts is given */
    int32_t *d_path_len;          /* [n]; required when starts is given */
} gg_plane_routes;
int gg_route_planes(gg_context *ctx, const gg_plane_routes *x, void *stream);
#define GG_HAS_ROUTE_PLANES 1

/* CORRELATIVE SCAN-TO-MAP MATCHING of many maps, in DEVICE memory: everything persistent in the chain above is placed by odometry the caller
 * hands in and nobody checks -- the map's own layers through gg_move_maps, the evidence of gg_fuse_states through the index shifts that
 * call returns -- and a shift that is one cell off smears every wall of the fused grid.  gg_match_planes scores this scan's occupied cells
 * against the accumulated grid over a window of translations and a few yaw candidates, and returns the best candidate and how ambiguous it
 * is.  What a caller otherwise composes per map from nonzero (which synchronises), a rotation, a scatter and a padded correlation per yaw.
 * Both inputs are planes of earlier calls as they stand.  Map i of the call is row i of every buffer and of `shifts` and `pivots`.
 * Everything is 32-bit integer; nothing wraps at the border; all of the following is per map:
 *   scan cell    cell (r, c) where map i's d_scan word is > 0 (a d_state plane of gg_visibility_clouds, a d_fused plane of gg_fuse_states:
 *                the occupied cells alone).
 *   reward       f(r, c) = min(max(word of d_field, 0), field_max) inside the map, 0 for any cell outside it (a d_evidence_out plane of
 *                gg_fuse_states as it stands: positive evidence means occupied; or a likelihood composed from a clearance plane).
 *   prior shift  (s0, s1) = (shifts[2 i], shifts[2 i + 1]), both 0 when `shifts` is NULL, WITH THE MEANING IT HAS IN gg_fuse_states: scan
 *                cell (r, c) lies over field cell (r + s0, c + s1).  Clamped to [-rows, rows] x [-cols, cols] as there.
 *   pivot        (pr, pc) = (pivots[2 i], pivots[2 i + 1]), a cell inside the map, (rows / 2, cols / 2) when `pivots` is NULL: the centre
 *                of rotation, the sensor's cell.
 *   rotation k   the pair (cq, sq) = (rotations[2 k], rotations[2 k + 1]) in Q14 (16384 = 1.0), shared by all maps, |cq|, |sq| <= 16384,
 *                1 <= n_rotations = K <= 64; NULL with n_rotations == 0 is the single candidate (16384, 0).  The pair is used as given: no
 *                unit length is asked for.  With dr = r - pr, dc = c - pc:  a = cq dr - sq dc,  b = sq dr + cq dc,  r' = pr + rnd(a),
 *                c' = pc + rnd(b), rnd(v) = (|v| + 8192) >> 14 with the sign of v: round half away from zero, the convention of
 *                gg_visibility_clouds.  rows, cols <= 32768 (GG_ERR_GEOMETRY), so a and b fit an int32.  The formula is in (row, col)
 *                terms and does not depend on `order`.  Two scan cells that land on the same (r', c') both count.
 *   score        S(k, dy, dx) = the sum over the scan cells of f(r' + s0 + dy, c' + s1 + dx), for every k and every translation (dy, dx) in
 *                [-W, W] x [-W, W] in (row, col) terms, W = `window`, 0 <= W <= 32.
 *   limits       field_max >= 1 and field_max * rows * cols <= 2^31 - 1: every score fits an int32.  The C ABI has no defaults.
 *   d_best[i]    six words: k*, dy*, dx*, S*, the number of scan cells of the map, and the number of candidates (k, dy, dx) whose score
 *                equals S*.  (k*, dy*, dx*) attains the maximum S*; among the maximisers it has the smallest dy^2 + dx^2, then the
 *                smallest k, then the smallest dy, then the smallest dx: a caller who lists the prior yaw first gets "no correction" on a
 *                featureless scene.  A map without scan cells gives (0, 0, 0, 0, 0, K (2 W + 1)^2).
 *   d_scores     nullable: map i's volume of K (2 W + 1)^2 words at d_scores + i * score_stride, S(k, dy, dx) at word
 *                (k (2 W + 1) + dy + W) (2 W + 1) + dx + W.  Every word of a given volume is written; the words between the volume and
 *                the stride never are.
 *   use          with k* the identity, (s0 + dy*, s1 + dx*) IS THE CORRECTED SHIFT TO PASS TO gg_fuse_states for this scan.  A k* that is
 *                not the identity is a yaw correction for the caller's next cloud-to-map transform; no call rotates planes.  The sixth
 *                word against K (2 W + 1)^2, and S* against field_max times the fifth, say how much to trust either.
 *   addressing   map i's plane of rows * cols int32 at d_scan + i * scan_stride and d_field + i * field_stride; cell (row, col) where
 *                `order` puts it, the same order for both planes.  4-byte alignment.
 *   no overlap   no output may share a byte with an input or with the other output; the call compares the address ranges as
 *                gg_route_planes does (a plane buffer from its first word to the last cell of its last plane, d_scores to the last word
 *                of its last volume) and answers GG_ERR_INVALID.  The two inputs may overlap each other.
 *   determinism  integer sums only: bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_fuse_states: NO MAP IS READ OR CHANGED -- no layer, position, freshness, configuration, score or liveness flag,
 * and the lazily kept layers stay pending.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry of the same ring of parameter entries
 * (the shifts, the pivots and the rotation table travel in it) and orders itself on `stream` as those calls do; it enqueues and returns with
 * no synchronisation, and the host arrays may be freed on return.  The caller's device buffers must stay valid and unmodified until
 * `stream` has passed the call.
 * Across streams the call is ordered, for the caller's buffers too, as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_scan, d_field or d_best, scan_stride or field_stride < rows * cols, score_stride < K (2 W + 1)^2 with d_scores given, an
 * unknown order, window outside [0, 32], field_max < 1 or beyond the limit, n_rotations outside [1, 64] with `rotations` given or != 0
 * without, a rotation word beyond +-16384, a pivot outside the map, overlapping buffers; GG_ERR_GEOMETRY for rows or cols > 32768;
 * GG_ERR_CAPACITY for n > n_slots.  n == 0 is GG_OK before anything else is looked at.  The first many-map call of a context may allocate
 * (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
#define GG_MATCH_MAX_WINDOW 32
#define GG_MATCH_MAX_ROTATIONS 64
#define GG_MATCH_UNIT 16384
typedef struct gg_plane_matches {
    int n;                        /* maps */
    const int32_t *d_scan;        /* [n] planes, scan_stride apart: a SCAN CELL where the word is > 0; required */
    size_t scan_stride;           /* int32 words, >= rows * cols */
    const int32_t *d_field;       /* [n] planes, field_stride apart: the reward min(max(word, 0), field_max); required */
    size_t field_stride;          /* int32 words, >= rows * cols */
    int field_max;                /* >= 1, field_max * rows * cols <= 2^31 - 1 */
    const int32_t *shifts;        /* host [n][2] prior shifts (rows, cols), as gg_state_fusion.shifts; NULL: all (0, 0) */
    const int32_t *pivots;        /* host [n][2] (row, col) inside the map; NULL: (rows / 2, cols / 2) for every map */
    const int32_t *rotations;     /* host [n_rotations][2] (cq, sq) in Q14; NULL with n_rotations == 0: the one candidate (16384, 0) */
    int n_rotations;              /* K, 1 .. 64 */
    int window;                   /* W, 0 .. 32 */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of both planes */
    int32_t *d_best;              /* [n][6]: k*, dy*, dx*, S*, scan cells, candidates that attain S*; required */
    int32_t *d_scores;            /* [n] volumes of K (2 W + 1)^2 int32, score_stride apart; nullable */
    size_t score_stride;          /* int32 words, >= K (2 W + 1)^2 when d_scores is given */
} gg_plane_matches;
int gg_match_planes(gg_context *ctx, const gg_plane_matches *x, void *stream);
#define GG_HAS_MATCH_PLANES 1

/* WHICH HEADINGS A VEHICLE FOOTPRINT FITS, per cell, for many maps in DEVICE memory: gg_route_planes blocks single cells, and the only size a
 * caller can give the robot there is one radius of inflation -- the circumscribed radius of a car closes every lane it fits through, the
 * inscribed one opens gaps it can only enter sideways.  gg_footprint_planes is the oriented-footprint test of a lattice planner: for every
 * cell and each of K headings, does the footprint placed at that cell with that heading touch a blocked cell?  What a caller otherwise
 * composes per map from K dense correlations with kernels of up to 65 x 65.  The input is a plane of an earlier call as it stands.  Map i of
 * the call is row i of every buffer.  Everything is 32-bit integer and in (row, col) terms whatever `order` is; all of the following is
 * per map:
 *   blocked      cell q is blocked where map i's d_blocked word is >= 0, as in gg_route_planes (a d_fused or d_state plane, a
 *                d_cell_cluster plane, a d_fit plane of this call as they stand).  Required.
 *   outside      a cell outside the map counts as blocked when outside_free == 0 and as free when outside_free == 1; no other value.
 *   footprint    K = n_headings (1 .. 32) headings and a radius R (0 .. 32) come with a HOST table spans[K][2 R + 1][2] of int32, shared by
 *                all maps of the call: row a + R of heading k holds (lo, hi), and the cells of heading k are
 *                F_k = {(a, b): -R <= a <= R, lo(k, a) <= b <= hi(k, a)}.  lo > hi is an empty row; a non-empty row needs
 *                -R <= lo <= hi <= R.  F_k must also be column-convex: for every b the rows a with (a, b) in F_k are consecutive
 *                (GG_ERR_INVALID otherwise; gg_footprint_spans makes such tables).  An empty F_k is allowed and fits everywhere.
 *   fits         heading k fits at (r, c) iff no cell (r + a, c + b) with (a, b) in F_k is blocked, the outside rule applied: the
 *                footprint is laid over the map, not reflected.
 *   d_mask       uint32 planes, nullable: bit k of the word of (r, c) is set iff heading k fits there; bits K .. 31 are zero.
 *   d_fit        int32 planes, nullable: with p = the number of headings that fit at the cell, the word is -1 where p >= min_fit and p
 *                (0 <= p < min_fit) elsewhere; 1 <= min_fit <= K.  A d_blocked plane of gg_route_planes and a seed plane of
 *                gg_clearance_clouds (d_seeds) as it stands.  min_fit == 1 is the exact projection of the configuration space ("fits at some
 *                heading"), min_fit == K the conservative one ("fits at every heading").
 *   d_counts     nullable: three words per map, d_counts[3 i + 0 .. 2]: the number of cells with p == K, with p >= min_fit, with p == 0.
 *   At least one of d_mask, d_fit and d_counts must be given.
 *   addressing   map i's plane of rows * cols words at d_blocked + i * blocked_stride, d_mask + i * mask_stride and d_fit + i * fit_stride;
 *                cell (row, col) where `order` puts it, the same order for all planes; strides >= rows * cols.  4-byte alignment.  Every
 *                cell of every given plane is written; the words between rows * cols and a stride never are.
 *   no overlap   no output may share a byte with the input or with another output; the call compares the address ranges as
 *                gg_route_planes does (a plane buffer from its first word to the last cell of its last plane, d_counts its 3 n words) and
 *                answers GG_ERR_INVALID.
 *   determinism  bit operations and integer sums only: bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_route_planes and gg_match_planes: NO MAP IS READ OR CHANGED -- no layer, position, freshness, configuration,
 * score or liveness flag, and the lazily kept layers stay pending.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry of the same
 * ring of parameter entries (the span table travels in it) and orders itself on `stream` as those calls do; it enqueues and returns with
 * no synchronisation, and the host table may be freed on return.  The caller's device buffers must stay valid and unmodified until
 * `stream` has passed the call.
 * Across streams the call is ordered, for the caller's buffers too, as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_blocked, null spans, no output at all, a stride < rows * cols, an unknown order, n_headings outside [1, 32], radius outside
 * [0, 32], min_fit outside [1, n_headings], outside_free not 0 or 1, a non-empty row with lo < -R or hi > R, a heading that is not
 * column-convex, overlapping buffers; GG_ERR_CAPACITY for n > n_slots.  n == 0 is GG_OK before anything else is looked at.  The first
 * many-map call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not
 * supported. */
#define GG_FOOTPRINT_MAX_HEADINGS 32
#define GG_FOOTPRINT_MAX_RADIUS 32
typedef struct gg_plane_footprints {
    int n;                        /* maps */
    const int32_t *d_blocked;     /* [n] planes, blocked_stride apart: BLOCKED where the word is >= 0; required */
    size_t blocked_stride;        /* int32 words, >= rows * cols */
    const int32_t *spans;         /* host [n_headings][2 radius + 1][2]: (lo, hi) of row a + radius; lo > hi: an empty row; required */
    int n_headings;               /* K, 1 .. 32 */
    int radius;                   /* R, 0 .. 32 */
    int min_fit;                  /* 1 .. K: d_fit is -1 where at least this many headings fit */
    int outside_free;             /* 0: cells outside the map are blocked, 1: they are free */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of all planes */
    uint32_t *d_mask;             /* [n] planes, mask_stride apart: bit k set iff heading k fits; nullable */
    size_t mask_stride;           /* words, >= rows * cols when d_mask is given */
    int32_t *d_fit;               /* [n] planes, fit_stride apart: -1 where p >= min_fit, else p; nullable */
    size_t fit_stride;            /* words, >= rows * cols when d_fit is given */
    int32_t *d_counts;            /* [n][3]: cells with p == K, with p >= min_fit, with p == 0; nullable */
} gg_plane_footprints;
int gg_footprint_planes(gg_context *ctx, const gg_plane_footprints *x, void *stream);

/* The span table of a RECTANGLE for gg_footprint_planes.  Host arithmetic only: no context, no device call.
 *   rotations    the Q14 table of gg_match_planes (GG_MATCH_UNIT = 1.0), [n_rotations][2], 1 <= n_rotations <= 32, |word| <= 16384: the
 *                forward axis of heading k is (cq, sq) = (rotations[2 k], rotations[2 k + 1]) in (row, col), used as given (no unit
 *                length is asked for).
 *   rect         (u_lo, u_hi, v_lo, v_hi) in units of 1/16384 cell, |word| <= 2^30, u_lo <= u_hi, v_lo <= v_hi: the extent along the
 *                forward axis and along the axis a quarter turn from it (the turn that takes the row axis to the column axis).
 *   membership   with u = cq a + sq b and v = -sq a + cq b (both fit an int32 for |a|, |b| <= 33), offset (a, b) belongs to heading k iff
 *                u_lo <= u <= u_hi and v_lo <= v <= v_hi.  This tests the centre of the cell: a caller who wants every cell the rectangle
 *                touches pads the rectangle.  Both conditions are intervals in b for a fixed a and in a for a fixed b, so every heading
 *                is row- and column-convex whatever the pair.
 *   needed       the test is evaluated on the box [-33, 33]^2.  *needed (nullable) receives the largest max(|a|, |b|) of a member cell
 *                over all headings, -1 when there is none; 33 means the footprint cannot be represented.
 *   spans        NULL: a pure query; `radius` is not looked at and the answer is GG_OK.  Otherwise 0 <= radius <= 32, and with
 *                needed <= radius the table [n_rotations][2 radius + 1][2] is written, row a + radius of heading k = (min b, max b) of
 *                its members, an empty row as (1, 0); with needed > radius the answer is GG_ERR_INVALID and `spans` is left untouched
 *                (*needed is written either way).
 * GG_ERR_INVALID also for null rotations or rect, n_rotations outside [1, 32], a rotation word beyond +-16384, a rect word beyond +-2^30,
 * lo > hi, and radius outside [0, 32] with `spans` given. */
int gg_footprint_spans(const int32_t *rotations, int n_rotations, const int32_t rect[4], int radius, int32_t *spans, int *needed);
#define GG_HAS_FOOTPRINT_PLANES 1

/* The NAVIGATION FUNCTION OF A STATE LATTICE, SE(2) on the grid, for many maps in DEVICE memory: gg_route_planes routes a point without a
 * heading, and gg_footprint_planes says at which headings a vehicle fits at a cell; the only way from one to the other is the d_fit
 * projection, which throws the headings away -- it does not know that a car cannot turn on the spot, has to back out of a dead end, or needs
 * room to swing round a corner.  gg_route_headings reads the heading mask: for every cell and every one of K headings it gives the exact cost D
 * of the cheapest chain of motion primitives ("moves") to a goal state, every state on the chain one the mask admits; the move to take, the
 * best heading per cell, three counts per map and, from one start pose per map, the path.  What a caller otherwise gets per map and per frame
 * from a download of the mask, a graph of (cell, heading) nodes, Dijkstra on the host and an upload.  Map i of the call is row i of every
 * buffer and of `starts`.  Everything is 32-bit integer and in (row, col) terms whatever `order` is; all of the following is per map:
 *   states       K = n_headings (1 .. 32).  A state is (k, q), heading k at cell q.  It is ADMISSIBLE where q lies inside the map and bit k of
 *                map i's d_mask word of q is set (a d_mask plane of gg_footprint_planes as it stands).  Bits K .. 31 are ignored.  Required.
 *   weight       w(q) = min(max(word of d_cost, 1), cost_max); 1 everywhere when d_cost is NULL: exactly as in gg_route_planes.
 *   moves        a HOST table moves[K][GG_HEADINGS_MAX_MOVES = 8][4] of int32, shared by all maps of the call: entry m of heading k is
 *                (da, db, k2, s).  s == 0 is an absent entry, whose other words are not looked at.  Otherwise 1 <= s <= 32767,
 *                |da|, |db| <= GG_HEADINGS_MAX_STEP = 3, 0 <= k2 < K, and not (da, db, k2) == (0, 0, k).  Turns in place (da = db = 0 with
 *                k2 != k) are allowed.  The move leads from (k, (r, c)) to (k2, (r + da, c + db)); it is admissible when both states are;
 *                it costs s * w of the cell ENTERED, (r + da, c + db), as in gg_route_planes.  The cells BETWEEN the two ends of a move
 *                longer than one cell are NOT looked at: the footprint table of gg_footprint_planes is where a caller covers them (a
 *                footprint padded by the length of the longest move sweeps every cell the vehicle passes over).  gg_heading_moves makes
 *                the table of a car-like vehicle.
 *   goals        (k, q) is a GOAL STATE when it is admissible, map i's d_goals word of q is >= 0 (a d_frontier plane of gg_fuse_states or
 *                a goal plane as for gg_route_planes, as it stands; required) and bit k of goal_headings is set.  0xFFFFFFFF means "any
 *                heading"; a goal_headings with none of its low K bits set means no goal state at all, which is legal.
 *   D            0 on a goal state; elsewhere the minimum, over all finite chains of admissible moves from (k, q) to a goal state, of the
 *                sum of the move costs; GG_ROUTE_NONE on an inadmissible state and where there is no such chain.  Equivalently D is the
 *                solution of D(k, q) = min over the admissible moves m of (k, q) of D(k2_m, q + d_m) + s_m * w(q + d_m) with D = 0 on the goal
 *                states and GG_ROUTE_NONE where the minimum is over nothing reached.  The solution is UNIQUE because every move costs at
 *                least 1: two solutions that differ would differ at a state of smallest value among those where they differ, whose
 *                minimising successor has a smaller value and so is equal in both -- a contradiction; hence D does not depend on how it
 *                is computed.
 *   limits       1 <= cost_max; max s (over the present moves) * cost_max * rows * cols * K <= 2^31 - 2, compared in 64 bits
 *                (GG_ERR_INVALID beyond).  A chain without a repeated state has fewer than rows * cols * K moves, so every true D fits an
 *                int32, every word the call stores while it works is <= 2^31 - 1 and one move costs <= 2^31 - 2: the UNSIGNED sum of a
 *                stored word and a move cannot wrap, which the kernel relies on.  The C ABI has no defaults.
 *   max_cost     R > 0: a state with D > R is reported as unreached (d_dist = GG_ROUTE_NONE, d_next = -1, not counted as reached, not a
 *                candidate of d_best); every other word is that of R = 0.  0: unbounded.
 *   d_dist       required, int32: K planes per map, plane k of map i at d_dist + i * dist_stride + k * plane_stride, plane_stride >=
 *                rows * cols and dist_stride >= K * plane_stride; cell (row, col) where `order` puts it.  d_dist[k][q] = D(k, q).  It is
 *                the call's working memory.
 *   d_next       nullable, int32, the same addressing with next_stride and next_plane_stride of its own: GG_HEADINGS_AT_GOAL (= 8) on a
 *                goal state, -1 where D is GG_ROUTE_NONE, otherwise the SMALLEST m whose admissible move attains the minimum.  Following
 *                it lowers D by at least 1 per move: every chain ends on a goal state and has no cycle.
 *   d_best, d_best_heading   nullable, one plane per map each at + i * best_stride / best_heading_stride: the minimum over k of D(k, q) and
 *                the SMALLEST k that attains it; GG_ROUTE_NONE and -1 where no heading of the cell is reached.  The plane a caller draws
 *                and compares with gg_route_planes'.
 *   d_counts[i]  nullable, three words per map: the number of goal states, of reached states (goal states included; under max_cost), and
 *                of admissible states.
 *   paths        with `starts`, a host array [n][2] of (cell, heading), cell a linear index in `order` or -1 for no start (the heading is
 *                then not looked at): map i's path is the start state, the state its d_next move leads to, ... up to and including the
 *                goal state.  d_paths holds rows of (cell, heading) pairs, path_stride words apart (>= 2 * max_len), at most max_len pairs
 *                each; d_path_len[i] is the number of states of the whole path, also when that exceeds max_len.  Pair j of row i is
 *                written for j < min(len, max_len) and the other words of the row never are.  The cell numbering, the unreached start
 *                (len 0, row untouched), the absent start and the truncation are exactly those of gg_route_planes' paths.  d_next need not
 *                be given for the paths.
 *   addressing   map i's plane of rows * cols words at d_mask + i * mask_stride, d_cost + i * cost_stride, d_goals + i * goal_stride; the
 *                same order for every plane of the call.  EVERY word of every given output plane inside rows * cols is written, of every
 *                map and heading; the words between rows * cols and a stride never are, and a NULL output is not touched.  4-byte
 *                alignment.
 *   no overlap   no output may share a byte with an input or with another output; the call compares the address ranges as
 *                gg_route_planes does (a buffer from its first word to the last cell of its last plane) and answers GG_ERR_INVALID.  The
 *                inputs may overlap each other.
 *   determinism  integer arithmetic only; D is a unique fixed point and d_next, d_best and the paths are functions of D: bit-identical
 *                from run to run and independent of scheduling.
 * The contract is that of gg_route_planes and gg_footprint_planes: NO MAP IS READ OR CHANGED -- no layer, position, freshness,
 * configuration, score or liveness flag, and the lazily kept layers stay pending.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry
 * of the same ring of parameter entries (the move table and the starts travel in it) and orders itself on `stream` as those calls do; it
 * enqueues and returns with no synchronisation, and the host arrays may be freed on return.  The caller's device buffers must stay valid
 * and unmodified until `stream` has passed the call.  One work-group computes one map's D, so many maps fill the device and a single map
 * runs on one compute unit.
 * Across streams the call is ordered, for the caller's buffers too, as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_mask, d_goals, d_dist or moves, n_headings outside [1, 32], a stride smaller than stated above for a given buffer, an
 * unknown order, cost_max < 1, max_cost < 0, a present move with s outside [1, 32767], |da| or |db| > 3, k2 outside [0, K) or (0, 0, k), a
 * product beyond the limit, `starts` given without d_paths, d_path_len, max_len >= 1 or path_stride >= 2 * max_len, a start cell < -1 or
 * >= rows * cols, a start heading outside [0, K) with a start cell >= 0, overlapping buffers; GG_ERR_CAPACITY for n > n_slots;
 * GG_ERR_GEOMETRY for a map of more than 4096 tiles (of 32 x 32 cells up to 16 headings, of 16 x 16 above).  n == 0 is GG_OK before anything
 * else is looked at.  The first many-map call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a
 * caller's graph is not supported. */
#define GG_HEADINGS_MAX 32
#define GG_HEADINGS_MAX_MOVES 8
#define GG_HEADINGS_MAX_STEP 3
#define GG_HEADINGS_MAX_COST 32767
#define GG_HEADINGS_AT_GOAL 8
typedef struct gg_heading_routes {
    int n;                        /* maps */
    const uint32_t *d_mask;       /* [n] planes, mask_stride apart: state (k, q) is admissible where bit k is set (a d_mask plane of
                                     gg_footprint_planes as it stands); required */
    size_t mask_stride;           /* words, >= rows * cols */
    const int32_t *d_cost;        /* [n] planes, cost_stride apart: w = min(max(word, 1), cost_max); NULL: w = 1 everywhere */
    size_t cost_stride;
    const int32_t *d_goals;       /* [n] planes, goal_stride apart: a goal cell where the word is >= 0; required */
    size_t goal_stride;
    uint32_t goal_headings;       /* bit k: heading k of a goal cell is a goal state; 0xFFFFFFFF: any heading */
    int n_headings;               /* K, 1 .. 32 */
    const int32_t *moves;         /* host [K][8][4]: (da, db, k2, s), s == 0 an absent entry; required */
    int cost_max;                 /* >= 1 */
    int max_cost;                 /* 0: unbounded; R > 0: a state whose D > R is reported as unreached */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    int32_t *d_dist;              /* [n][K] planes; required: the call's working memory */
    size_t dist_stride;           /* between maps, >= K * plane_stride */
    size_t plane_stride;          /* between the headings of a map, >= rows * cols */
    int32_t *d_next;              /* [n][K] planes; nullable */
    size_t next_stride;           /* >= K * next_plane_stride when d_next is given */
    size_t next_plane_stride;     /* >= rows * cols when d_next is given */
    int32_t *d_best;              /* [n] planes, best_stride apart: min over k of D; nullable */
    size_t best_stride;
    int32_t *d_best_heading;      /* [n] planes, best_heading_stride apart: the smallest k that attains it, -1: none; nullable */
    size_t best_heading_stride;
    int32_t *d_counts;            /* [n][3]: goal states, reached states (goal states included), admissible states; nullable */
    const int32_t *starts;        /* host [n][2]: (linear index in `order` of the start cell or -1, heading); nullable */
    int32_t *d_paths;             /* [n] rows of (cell, heading) pairs, path_stride words apart; required when starts is given */
    size_t path_stride;           /* words, >= 2 * max_len */
    int max_len;                  /* pairs of a row, >= 1 when starts is given */
    int32_t *d_path_len;          /* [n]; required when starts is given */
} gg_heading_routes;
int gg_route_headings(gg_context *ctx, const gg_heading_routes *x, void *stream);

/* The move table of a CAR-LIKE vehicle for gg_route_headings.  Host arithmetic only: no context, no device call.
 *   rotations    the Q14 table of gg_match_planes / gg_footprint_spans, [n_rotations][2], 1 <= n_rotations = K <= 32, |word| <= 16384: the
 *                forward axis of heading k is (cq, sq) in (row, col), used as given.
 *   step         L in 1 .. 3: the length of a translating move in cells.  d_k = (rha(L * cq), rha(L * sq)) with rha(v) = (|v| + 8192) >> 14
 *                with the sign of v: L * cq / 16384 rounded half away from zero, the convention of gg_match_planes.
 *   unit         U in 1 .. 1024: the cost of one cell of travel.  s_k = max(1, floor(sqrt(U * U * (da^2 + db^2)))), an exact integer root.
 *   turn         >= 0, added to a move that changes the heading by one.
 *   reverse_pct  0: no reverse moves; otherwise >= 100: a reverse move costs ceil(cost * reverse_pct / 100) of its forward twin.
 *   spin         >= 0: the cost of a turn in place by one heading; 0: none.
 *   moves        [K][8][4] is written, heading k:  slot 0 (d_k, k, s_k);  1 (d_k, (k + 1) mod K, s_k + turn);  2 (d_k, (k - 1) mod K,
 *                s_k + turn);  3 .. 5 the same three with -d_k and the reverse cost, absent with reverse_pct == 0;  6 and 7
 *                (0, 0, (k + 1) mod K, spin) and (0, 0, (k - 1) mod K, spin), absent with spin == 0 or K == 1.  A heading with d_k == (0, 0)
 *                gets no translating moves.  An absent entry is four zeros.
 * GG_ERR_INVALID, with `moves` untouched, for null rotations or moves, a range violation above, a rotation word beyond +-16384, and a cost
 * above 32767. */
int gg_heading_moves(const int32_t *rotations, int n_rotations, int step, int unit, int turn, int reverse_pct, int spin, int32_t *moves);
#define GG_HAS_ROUTE_HEADINGS 1

/* WHICH OBJECT IS WHICH, for many maps in DEVICE memory: gg_cluster_clouds numbers the clusters of ONE scan by their smallest cell, so the
 * same car is cluster 17 in one frame and cluster 4 in the next.  gg_track_clusters is the data association of this scan's clusters with the
 * last scan's: it counts, for every pair of a current and a previous cluster, the cells of the one that lie on (or within `gate` cells of)
 * the other once the previous plane is shifted by what gg_move_maps returned, lets every current cluster name its best predecessor and every
 * predecessor keep its best claimant, and hands down a PERSISTENT track id, an age and the overlap figures; clusters without a predecessor
 * get fresh ids.  What a caller otherwise gets per map and per frame from a download of two id planes, a contingency table on the host and
 * an upload.  Map i of the call is row i of every buffer and of `shifts`.  Everything is 32-bit integer and in (row, col) terms whatever
 * `order` is; with M = max_clusters, g = gate and (s0, s1) = (shifts[2 i], shifts[2 i + 1]) (both 0 when `shifts` is NULL), per map:
 *   clusters     Kc = min(1 + the largest word of the current plane, M), 0 for a plane without a word >= 0.  A cell whose word is < 0 or >= M
 *                belongs to no cluster (a d_cell_cluster plane of gg_cluster_clouds as it stands: -1 or the id).  Kp = min(max(heads_in[1],
 *                0), M), heads_in being map i's four words of d_heads_in; a previous cell whose word is < 0 or >= Kp holds nothing.  WITHOUT
 *                A PRIOR (d_cells_prev, d_tracks_in and d_heads_in all NULL) Kp = 0 and next_id = 0; otherwise next_id = heads_in[0].
 *   overlap      O[c][p] = the number of pairs (cell (r, q) of current cluster c, offset (a, b) in [-g, g]^2) such that (r + s0 + a,
 *                q + s1 + b) lies inside the map and the previous plane holds p there.  THE SHIFT HAS THE MEANING IT HAS IN gg_fuse_states:
 *                current cell (r, q) lies over previous cell (r + s0, q + s1); nothing wraps.  From |s0| >= rows or |s1| >= cols on O is 0
 *                everywhere, whatever the gate.  S[c][p] counts the pairs with (a, b) = (0, 0) alone.
 *   candidate    p*(c) = the p with the largest O[c][p] > 0, the smallest such p among equals; undefined when row c of O is 0.
 *   winner       of p: among the c with p*(c) = p the one with the largest O[c][p], the smallest such c among equals.
 *   inheritance  c CONTINUES p*(c) iff it is that p's winner: prev = p, track_id = tracks_in[p].track_id, age = min(tracks_in[p].age,
 *                INT32_MAX - 1) + 1, overlap = O[c][p], still = S[c][p].  tracks_in is map i's row of d_tracks_in, M records long.  Of a
 *                SPLIT the part with the larger overlap keeps the track and the others are new; a MERGE ends the tracks that lost.
 *   birth        every other cluster is new: prev = -1, overlap = still = 0, age = 0, track_id = (next_id + j) & 0x7FFFFFFF with j its rank
 *                among the new clusters in ascending c.
 *   records      d_tracks_out[i][k], k < Kc, describes cluster k of THIS scan: the above and cells, sum_row, sum_col over its cells (the
 *                centroid is sum / cells).  Records k >= Kc are never written.
 *   heads        d_heads_out[i] = {(next_id + born) & 0x7FFFFFFF, Kc, born, ended}: born = the new clusters, ended = Kp - the inheriting
 *                ones.  The four words are what the next call takes as d_heads_in, with d_tracks_out as d_tracks_in and d_cells as
 *                d_cells_prev: the caller alternates between two id planes and two record buffers.
 *   d_cell_track nullable: the track id of the cell's cluster, -1 on a cell of no cluster.  Every cell inside rows * cols is written.
 *   limits       1 <= M <= GG_TRACK_MAX_CLUSTERS = 1024; 0 <= g <= 4; rows * cols * max(rows, cols) <= 2^31 - 1 (GG_ERR_GEOMETRY beyond), so
 *                the coordinate sums and O (<= 81 rows * cols) stay inside an int32.
 *   addressing   map i's plane of rows * cols int32 at d_cells + i * cells_stride, d_cells_prev + i * prev_stride, d_cell_track + i *
 *                track_stride; cell (row, col) where `order` puts it, the same order for every plane of the call.  The words between
 *                rows * cols and a stride are never written, and a NULL output is not touched.  4-byte alignment.
 *   no overlap   no output may share a byte with an input or with another output; the call compares the address ranges as gg_fuse_states
 *                does and answers GG_ERR_INVALID.  The inputs may overlap each other.
 *   determinism  integer arithmetic and integer atomics only (adds, and maxima of keys that differ): the result is a function of the
 *                inputs alone, bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_fuse_states: NO MAP IS READ OR CHANGED -- no layer, position, freshness, configuration, score or liveness flag,
 * and the lazily kept layers stay pending; the tracks live in the caller's buffers, not in the context.  n <= n_slots (GG_ERR_CAPACITY):
 * the call takes an entry of the same ring of parameter entries (the shifts travel in it) and orders itself on `stream` as that call does;
 * it enqueues and returns, and `shifts` may be freed on return.  The caller's device buffers must stay valid and unmodified until `stream`
 * has passed the call.  One work-group computes one map, so many maps fill the device and a single map runs on one compute unit.
 * Across streams the call is ordered, for the caller's buffers too, as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_cells, d_tracks_out or d_heads_out, only some of d_cells_prev, d_tracks_in and d_heads_in given, cells_stride < rows * cols,
 * prev_stride < rows * cols with a prior, track_stride < rows * cols with d_cell_track, an unknown order, max_clusters outside [1, 1024], gate
 * outside [0, 4], overlapping buffers; GG_ERR_CAPACITY for n > n_slots; GG_ERR_GEOMETRY for a map beyond the limit above.  n == 0 is GG_OK
 * before anything else is looked at.  The first many-map call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.
 * Capture into a caller's graph is not supported. */
#define GG_TRACK_MAX_CLUSTERS 1024
typedef struct gg_track {      /* 32 bytes: record k describes cluster k of THIS scan */
    int32_t track_id;          /* persistent id: inherited, or newly given */
    int32_t age;               /* 0 for a new track, the predecessor's age + 1 otherwise (saturating) */
    int32_t prev;              /* cluster index in the previous scan it continues, or -1 */
    int32_t overlap;           /* O[k][prev], 0 when prev == -1 */
    int32_t still;             /* the offset-(0,0) part of overlap: cells that lie exactly on the predecessor */
    int32_t cells;             /* cells of cluster k */
    int32_t sum_row, sum_col;  /* sums of (row, col) over its cells: centroid = sum / cells */
} gg_track;
typedef struct gg_cluster_tracks {
    int n;                        /* maps */
    const int32_t *d_cells;       /* [n] id planes of this scan, cells_stride apart (gg_cluster_clouds' d_cell_cluster as it stands); required */
    size_t cells_stride;          /* int32 words, >= rows * cols */
    const int32_t *d_cells_prev;  /* [n] id planes of the previous scan, prev_stride apart; NULL: no prior */
    size_t prev_stride;           /* >= rows * cols with a prior */
    const gg_track *d_tracks_in;  /* [n][max_clusters]: the previous call's d_tracks_out; NULL: no prior */
    const int32_t *d_heads_in;    /* [n][4]: the previous call's d_heads_out; NULL: no prior */
    const int32_t *shifts;        /* host [n][2] index shifts (rows, cols) as gg_fuse_states takes them; NULL: all (0, 0) */
    int max_clusters;             /* M, 1 .. GG_TRACK_MAX_CLUSTERS */
    int gate;                     /* g, 0 .. 4 cells */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    gg_track *d_tracks_out;       /* [n][max_clusters]; required */
    int32_t *d_heads_out;         /* [n][4]: next_id, clusters, born, ended; required */
    int32_t *d_cell_track;        /* [n] planes, track_stride apart: the cell's track id, -1 elsewhere; nullable */
    size_t track_stride;          /* >= rows * cols with d_cell_track */
} gg_cluster_tracks;
int gg_track_clusters(gg_context *ctx, const gg_cluster_tracks *x, void *stream);
#define GG_HAS_TRACK_CLUSTERS 1

/* THE SHAPE OF AN OBJECT, for the clusters of many clouds in DEVICE memory: a gg_cluster has an axis-aligned cell box and a gg_track a cell
 * centroid, and on 0.33 m cells neither says which way a car points, how long and wide it is or where its centre lies.  gg_box_clusters fits
 * a search-based rectangle to every cluster: for each of up to 32 candidate headings the extent of the cluster's points along and across the
 * heading, the heading chosen by an integer criterion, one 32-byte record per cluster.  What a caller otherwise gets from a download of the
 * per-point ids and the points, or from one scatter_reduce per heading and per map.  It runs right behind gg_cluster_clouds on that call's
 * points, d_point_cluster and d_n_clusters, and reads no layer.  One call for many maps; cloud i meets map slots ? slots[i] : first_slot + i
 * (distinct, inside the context).  All arithmetic is integer after one quantisation step; with M = max_clusters and K = n_rotations:
 *   clusters     M_i = min(max(d_n_clusters[i], 0), M), read on the device.
 *   participation  point p < n_points[i] of cloud i participates when (1) its id d_point_cluster[i][p] lies in [0, M_i) and (2) its
 *                map-frame position lies inside its map under the map's current position, by the path's own inside test (:222-231) -- with
 *                `transforms` tested on the map-frame point the path computes (tf2::doTransform in double, cast to float), as
 *                gg_cluster_clouds has it.  Any other id, any coordinates (NaN, inf) and any d_n_clusters word are memory-safe and select
 *                nothing.
 *   quantisation GG_BOX_UNIT = 16 units per cell: ux = (int32_t)floor(((double)px - pos_x) * s) and uy likewise from py and pos_y, with
 *                s = 16.0 / resolution computed once on the host in double from the resolution the inside test uses; (pos_x, pos_y) is the
 *                map's position.  A subtraction, then a multiplication: nothing can be contracted.  A map with more than 4096 rows or
 *                columns is GG_ERR_GEOMETRY, so |u| <= 8 * side + 1 <= 32769.
 *   headings     `rotations` is a host table [K][2] of Q14 pairs (cq, sq) = (16384 cos, 16384 sin), the table gg_match_planes takes;
 *                1 <= K <= GG_BOX_MAX_HEADINGS = 32 and every word lies in [-16384, 16384].  For a rectangle the caller lists angles in
 *                [0, pi/2).  The projections of a point are a = ux * cq + uy * sq and b = uy * cq - ux * sq; both fit an int32
 *                (32769 * 32768 < 2^31).
 *   extents      per cluster c and heading k: a_min, a_max, b_min, b_max over the participating points with id c; A = a_max - a_min and
 *                B = b_max - b_min are taken in 64 bits (they can reach 2^31 + 2^16).
 *   criterion    GG_BOX_AREA: cost[c][k] = A * B, the minimum-area rectangle.  GG_BOX_EDGE: cost[c][k] = the sum over the cluster's
 *                participating points of min(a - a_min, a_max - a, b - b_min, b_max - b), the closeness criterion of L-shape fitting: the
 *                points of a car seen from one corner hug two edges of the right rectangle.  Both are uint64 and cannot overflow
 *                (A * B < 2^63; the sum stays below 2^31 * 2^24).
 *   choice       k* = the heading with the smallest cost, the smallest k among equals: a cluster of one point takes heading 0.
 *   d_boxes[i][c]  for c < M_i, every field: heading = k*, points = its participating points, the four extents at k*, and the cost at k* as
 *                two words.  A cluster c < M_i without a participating point gets heading = -1 and zeros.  Records at and beyond M_i are
 *                never written.
 *   d_costs      nullable, uint64 [n][M][K]: every cost[c][k] for c < M_i, all ones (UINT64_MAX) for a cluster without a participating
 *                point; never written from M_i on.  The ambiguity measure of a square-ish cluster.  8-byte alignment.
 *   no overlap   no output may share a byte with an input or with another output (GG_ERR_INVALID).  The inputs may overlap each other.
 *   determinism  integer arithmetic and integer atomics (min, max, add) only, no float is ever added: the result is a function of the
 *                inputs alone, bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_split_clouds, minus the labels: the call reads the caller's buffers and the maps' positions and NO LAYER; a
 * fresh map stays fresh; no layer, position, configuration, score or liveness flag changes and the lazily kept layers stay pending.
 * `stream`, ordering and the lifetime of the host arrays (slots, n_points, transforms, rotations: free on return) are those of
 * gg_split_clouds.  One work-group computes one cloud, so many clouds fill the device and a single cloud runs on one compute unit.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: every error of gg_cloud_clusters' members of the same name (null d_points or n_points, an unknown point_format, a bad slot list,
 * n_points[i] < 0 or > cloud_stride; GG_ERR_CAPACITY beyond max_points), null d_point_cluster, d_n_clusters, d_boxes or rotations,
 * n_rotations outside [1, 32], a rotation word outside [-16384, 16384], an unknown criterion, max_clusters outside [1, 4096], overlapping
 * buffers; GG_ERR_GEOMETRY for a map of more than 4096 rows or columns (no kernel is launched; gg_create refuses such a map today, its own
 * limits end below that side, so the bound is the call's arithmetic stated, not a case a context can reach).  n == 0 is GG_OK before anything else is
 * looked at.  The first call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph
 * is not supported. */
#define GG_BOX_UNIT 16
#define GG_BOX_MAX_HEADINGS 32
#define GG_BOX_MAX_CLUSTERS 4096
enum { GG_BOX_AREA = 0, GG_BOX_EDGE = 1 };
typedef struct gg_box {            /* 32 bytes: record c describes cluster c of the cloud */
    int32_t heading;               /* k*, the index into `rotations`; -1: no participating point */
    int32_t points;                /* participating points of the cluster */
    int32_t a_min, a_max;          /* the extent along heading k*, in Q14 units of GG_BOX_UNIT-ths of a cell */
    int32_t b_min, b_max;          /* ... and across it */
    int32_t cost_lo, cost_hi;      /* the uint64 cost at k*, low word first */
} gg_box;
typedef struct gg_cluster_boxes {
    int n;                         /* clouds */
    int first_slot;                /* cloud i meets map first_slot + i when slots == NULL */
    const int32_t *slots;          /* host [n], nullable, distinct */
    int point_format;              /* GG_POINT32 / GG_POINT16 */
    const void *d_points;          /* [n][cloud_stride], as gg_batch.d_points */
    size_t cloud_stride;           /* points */
    const int32_t *n_points;       /* host [n] */
    const double *transforms;      /* host [n][12], nullable, as gg_batch.transforms */
    const int32_t *d_point_cluster; /* [n][cloud_stride]: gg_cluster_clouds' d_point_cluster as it stands; required */
    const int32_t *d_n_clusters;   /* [n]: gg_cluster_clouds' d_n_clusters as it stands; required */
    const int32_t *rotations;      /* host [n_rotations][2] Q14 pairs (cq, sq); required */
    int n_rotations;               /* K, 1 .. GG_BOX_MAX_HEADINGS */
    int criterion;                 /* GG_BOX_AREA / GG_BOX_EDGE */
    int max_clusters;              /* M, 1 .. GG_BOX_MAX_CLUSTERS */
    gg_box *d_boxes;               /* [n][max_clusters]; required */
    uint64_t *d_costs;             /* [n][max_clusters][n_rotations], nullable */
} gg_cluster_boxes;
int gg_box_clusters(gg_context *ctx, const gg_cluster_boxes *x, void *stream);
#define GG_HAS_BOX_CLUSTERS 1

/* THE SCORE OF CANDIDATE TRAJECTORIES of many maps in DEVICE memory: gg_route_headings ends with the exact cost-to-go D(k, q) of every
 * (cell, heading) state, and all a caller can do with it on the device is read one d_next chain per map.  A local planner (the arc library
 * of a DWA or state-lattice planner, the sampled rollouts of MPPI) samples hundreds to thousands of short motions from the robot's pose
 * and has to throw away those that touch something, score the rest by what they cost plus what is left to go at their end, and pick one.
 * gg_score_rollouts does that on the planes the chain already holds: the heading mask of gg_footprint_planes, the cost plane, the D volume
 * of gg_route_headings and a squared-distance plane of gg_clearance_clouds in plane mode (`clearance_planes` in api.py), each as it stands.
 * What a caller otherwise gets from a download
 * of K + 2 planes per map, or in torch from index arithmetic, three gathers, a cumprod and a cumsum over [maps, rollouts, steps] tensors.
 * Map i of the call is row i of every buffer and of `starts`.  Everything is 32-bit integer unless 64 bits are named, and in (row, col)
 * terms whatever `order` is; all of the following is per map:
 *   headings     K = n_headings (1 .. 32).
 *   start        `starts`, a HOST array [n][3] of (r16, c16, k0): the robot's position in units of 1/16 cell (16 * row + 8 is the centre of a
 *                cell; GG_BOX_UNIT = 16 units per cell as in gg_box_clusters) and its heading.  0 <= r16 < 16 * rows, 0 <= c16 < 16 * cols,
 *                0 <= k0 < K.  r16 == -1: the map has no start, and the other two words are not looked at.  The start state is NOT tested
 *                against the mask: the robot is where it is.  Required.
 *   table        d_table, a DEVICE buffer of int32: entry (t, p), step t < T = n_steps of rollout p < P = n_rollouts, is the four words
 *                (da, db, dk, s) at d_table + i * table_stride + (t * P + p) * 4 -- step-major, so that consecutive rollouts are
 *                consecutive in memory.  table_stride == 0: one table shared by all maps (an arc library); otherwise >= 4 * P * T words
 *                (per-map samples).  1 <= P <= GG_ROLLOUTS_MAX = 65536, 1 <= T <= GG_ROLLOUTS_MAX_STEPS = 128.  The table is device data
 *                and is NOT validated: every possible word has a meaning below, and no word makes the call read or write outside its
 *                buffers.  Required.
 *   len          len_p is the smallest t with s(t, p) <= 0, or T.  Entries at and behind it are not looked at.
 *   pose t < len under frame == GG_ROLLOUTS_RELATIVE, with (cq, sq) the Q14 pair of heading k0 of the HOST table rotations[K][2] (the
 *                table of gg_match_planes / gg_heading_moves, |word| <= 16384, used as given, required in this frame):
 *                A = cq * da - sq * db and B = sq * da + cq * db, both in 64 bits; r16_t = r16 + rha(A), c16_t = c16 + rha(B) with
 *                rha(v) = (|v| + 8192) >> 14 with the sign of v -- the rotation of gg_match_planes: the offset (1, 0) goes to the forward
 *                axis; k_t = (k0 + dk) mod K, taken in [0, K) for any dk.
 *                Under GG_ROLLOUTS_ABSOLUTE: (r16_t, c16_t) = (da, db) and k_t = dk mod K in [0, K); rotations may be NULL.
 *                The pose's cell is (floor(r16_t / 16), floor(c16_t / 16)), flooring towards minus infinity.
 *   admissible   a pose is, when its cell lies inside the map -- with reach = R > 0 also within R rows and R columns of the start's
 *                cell -- and bit k_t of the cell's word of map i's d_mask plane is set (a d_mask plane of gg_footprint_planes as it
 *                stands; required).  The cells BETWEEN consecutive poses are not looked at, as in gg_route_headings: pad the footprint.
 *   step cost    min(s, 32767) * w(cell) with w = min(max(word of d_cost, 1), cost_max), 1 when d_cost is NULL: exactly gg_route_planes'.
 *   d_records    eight int32 per rollout, record p of map i at d_records + i * record_stride + 8 * p, record_stride >= 8 * P words:
 *                  0 steps        the number of leading admissible poses
 *                  1 len          len_p
 *                  2 cost         the sum of the step costs of poses 0 .. steps - 1
 *                  3 end_cell     the linear index in `order` of the cell of pose steps - 1; the start's cell when steps == 0
 *                  4 end_heading  k of pose steps - 1; k0 when steps == 0
 *                  5 togo         when the rollout is COMPLETE (steps == len): the word D(end_heading, end_cell) of d_dist, 0 when d_dist
 *                                 is NULL; GG_ROUTE_NONE when it is not complete.  d_dist is the [n][K] volume of gg_route_headings as it
 *                                 stands, plane k of map i at d_dist + i * dist_stride + k * plane_stride, plane_stride >= rows * cols,
 *                                 dist_stride >= K * plane_stride.
 *                  6 clear        the signed minimum of the d_clear words over poses 0 .. steps - 1 (d_clear: a d_dist2 plane of
 *                                 gg_clearance_clouds in plane mode (`clearance_planes` in api.py) as it stands, clear_stride >=
 *                                 rows * cols); GG_ROUTE_NONE when d_clear is NULL or steps == 0.
 *                  7 total        min(cost + togo, GG_ROUTE_NONE - 1), taken in 64 bits, when the rollout is complete,
 *                                 togo != GG_ROUTE_NONE and togo >= 0; GG_ROUTE_NONE otherwise.
 *                A rollout with len == 0 is complete: it stands for "stay", its end is the start state.  A map without a start gets
 *                (0, 0, 0, -1, -1, NONE, NONE, NONE) in every record.
 *   d_best[i]    nullable, four words per map: the smallest p that attains the least total among the rollouts with total !=
 *                GG_ROUTE_NONE, or -1 when there is none; that total, or GG_ROUTE_NONE; the number of complete rollouts; the number of
 *                rollouts with total != GG_ROUTE_NONE.  (-1, GG_ROUTE_NONE, 0, 0) for a map without a start.
 *   limit        cost_max >= 1 and T * 32767 * cost_max <= 2^31 - 2, compared in 64 bits (GG_ERR_INVALID beyond): `cost` never wraps.
 *   writes       every record p < P of every map is written; the words between 8 * P and record_stride never are; a NULL d_best is not
 *                touched.  4-byte alignment (the kernel takes 16-byte accesses where a row's address allows them).
 *   no overlap   neither output may share a byte with an input or with the other output; the call compares the address ranges as
 *                gg_route_headings does (d_table: 4 * P * T words, of the last map's table when table_stride > 0) and answers
 *                GG_ERR_INVALID.  The inputs may overlap each other.
 *   determinism  integer arithmetic only; a record is a function of its rollout and the best of a map a minimum of distinct keys:
 *                bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_route_headings: NO MAP IS READ OR CHANGED.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry of the
 * same ring of parameter entries (the starts and the rotation table travel in it) and orders itself on `stream` as those calls do; it
 * enqueues and returns with no synchronisation, and the host arrays may be freed on return.  The caller's device buffers must stay valid
 * and unmodified until `stream` has passed the call.  One work-group scores one map's rollouts, so many maps fill the device and a single
 * map runs on one compute unit.  Across streams the call is ordered as gg_state_fusion has it: ORDER OF THE MANY-MAP CALLS ACROSS STREAMS.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx, null x, n < 0; and with n > 0: null d_mask, d_table,
 * d_records or starts, null rotations in the relative frame, n_headings outside [1, 32], n_rollouts outside [1, 65536], n_steps outside
 * [1, 128], an unknown frame or order, reach outside [0, GG_ROLLOUTS_MAX_REACH = 63], a stride smaller than stated above for a given
 * buffer, table_stride in (0, 4 * P * T), a rotation word beyond +-16384 (relative frame), a start out of range, cost_max < 1 or a product
 * beyond the limit, overlapping buffers; GG_ERR_CAPACITY for n > n_slots.  n == 0 is GG_OK before anything else is looked at.  The first
 * many-map call of a context may allocate (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not
 * supported. */
#define GG_ROLLOUTS_MAX 65536
#define GG_ROLLOUTS_MAX_STEPS 128
#define GG_ROLLOUTS_MAX_REACH 63
#define GG_ROLLOUTS_RECORD_WORDS 8
enum { GG_ROLLOUTS_RELATIVE = 0, /* table entries are offsets in the start pose's frame, rotated by heading k0 */
       GG_ROLLOUTS_ABSOLUTE = 1 }; /* table entries are positions in 1/16 cell and headings */
typedef struct gg_rollouts {
    int n;                        /* maps */
    const uint32_t *d_mask;       /* [n] planes, mask_stride apart: pose (k, q) is admissible where bit k is set; required */
    size_t mask_stride;           /* words, >= rows * cols */
    const int32_t *d_cost;        /* [n] planes, cost_stride apart: w = min(max(word, 1), cost_max); NULL: w = 1 everywhere */
    size_t cost_stride;
    const int32_t *d_dist;        /* [n][K] planes of gg_route_headings; NULL: togo = 0 */
    size_t dist_stride;           /* between maps, >= K * plane_stride when d_dist is given */
    size_t plane_stride;          /* between the headings of a map, >= rows * cols when d_dist is given */
    const int32_t *d_clear;       /* [n] planes, clear_stride apart: squared distances; nullable */
    size_t clear_stride;
    int n_headings;               /* K, 1 .. 32 */
    const int32_t *starts;        /* host [n][3]: (r16, c16, k0); r16 == -1: no start; required */
    const int32_t *rotations;     /* host [K][2] Q14 (cq, sq); required in the relative frame */
    int frame;                    /* GG_ROLLOUTS_RELATIVE / GG_ROLLOUTS_ABSOLUTE */
    const int32_t *d_table;       /* (da, db, dk, s) of entry (t, p) at + i * table_stride + (t * P + p) * 4; required */
    size_t table_stride;          /* 0: one table for all maps; otherwise >= 4 * P * T words */
    int n_rollouts;               /* P, 1 .. GG_ROLLOUTS_MAX */
    int n_steps;                  /* T, 1 .. GG_ROLLOUTS_MAX_STEPS */
    int cost_max;                 /* >= 1; n_steps * 32767 * cost_max <= 2^31 - 2 */
    int reach;                    /* 0: the whole map; R in 1 .. 63: poses within R rows and R columns of the start's cell */
    int order;                    /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    int32_t *d_records;           /* [n] rows of P records of eight words, record_stride apart; required */
    size_t record_stride;         /* words, >= 8 * P */
    int32_t *d_best;              /* [n][4]: best p, its total, complete rollouts, scored rollouts; nullable */
} gg_rollouts;
int gg_score_rollouts(gg_context *ctx, const gg_rollouts *x, void *stream);
#define GG_HAS_SCORE_ROLLOUTS 1

/* The CONNECTED REGIONS OF ANY PLANE of many maps in DEVICE memory: gg_cluster_clouds labels only the occupancy it rasterises itself from
 * one scan's points, and every later link of the chain works on planes the caller already holds -- the state plane of gg_visibility_clouds,
 * the fused and frontier planes of gg_fuse_states, the fit plane of gg_footprint_planes, the D plane of gg_route_planes.  gg_cluster_planes
 * labels the connected components of the cells of such a plane whose word lies in a range, drops the components of fewer than min_cells
 * cells, and gives the plane of ids, the plane of component sizes, four counts per map and a table of the regions with their centroid sums
 * and the minimum of a second plane over every region: frontier regions ranked by size and by how far away they are, the persistent
 * objects of a fused grid for gg_track_clusters, and the despeckling of a costmap.  What a caller otherwise gets from a download,
 * scipy.ndimage.label + bincount + a relabel per map on the host and an upload.  Map i of the call is row i of every buffer.  Everything
 * is integer and in (row, col) terms whatever `order` is; L is the linear cell index of `order` (r * cols + c for GG_PLANES_ROWMAJOR,
 * r + c * rows for GG_PLANES_COLMAJOR), as in gg_cluster_clouds; per map:
 *   member       a cell of the plane at d_seeds + i * seed_stride whose int32 word w satisfies lo <= w <= hi.  lo = 0, hi = INT32_MAX is the
 *                ">= 0" rule of gg_clearance_clouds' seeds (a frontier plane, an id plane, "occupied or unknown" of a state plane);
 *                lo = hi = 1 selects the occupied cells of a state plane and lo = hi = -1 its free space.
 *   component    a connected component of members under `connectivity` 4 or 8, with the neighbours of gg_cluster_clouds: nothing wraps
 *                at the border.  Its size is its number of cells.
 *   kept         a component is kept when its size is at least min_cells (>= 1); the others are dropped.
 *   numbering    the kept components of a map are numbered 0 .. K-1 in ascending order of their smallest L.
 *   d_cell_cluster  required, and the call's working memory: map i's plane of rows * cols int32 at d_cell_cluster + i * plane_stride.
 *                EVERY cell inside rows * cols is written: -1 on a non-member and on a cell of a dropped component, else the id.  The
 *                plane is a d_cells plane of gg_track_clusters and a seed plane of gg_clearance_clouds as it stands.  The words between
 *                rows * cols and plane_stride are never written.  While the call runs the planes hold intermediate words.
 *   d_cell_size  nullable when min_cells == 1, required otherwise: the working memory of the filter.  Every cell inside rows * cols of
 *                the plane at d_cell_size + i * size_stride is written: 0 on a non-member, else the size of the cell's component -- on
 *                the cells of a dropped component too, so the caller sees what was removed.
 *   d_heads[i]   nullable, four int32: {K, dropped components, member cells, kept cells}, true counts also when K > max_regions.
 *   d_regions[i][k]  nullable: gg_region records of 48 bytes, written for k < min(K, max_regions), every field; records at and beyond
 *                that never are.  cells, the four bounds and first_cell (the region's smallest L) as in gg_cluster; sum_row and sum_col
 *                are the int64 sums of (row, col) over its cells: centroid = sum / cells.  8-byte alignment.
 *   d_values     a nullable int32 plane per map at d_values + i * value_stride; D of gg_route_planes plugs in as it stands.  value_min
 *                is the minimum of the plane over the region's cells as a signed int32, value_cell the L of the cell that attains it,
 *                the smallest L among equals.  Without d_values value_min = INT32_MAX and value_cell = -1.  (While the call runs the two
 *                words hold one 64-bit key, (value ^ 0x80000000) << 32 | L: that is what their order is for.)
 *   addressing   cell (row, col) where `order` puts it, the same order for every plane of the call.  4-byte alignment of the planes.
 *   no overlap   no output may share a byte with an input or with another output; the call compares the address ranges as
 *                gg_fuse_states does and answers GG_ERR_INVALID.  The inputs may overlap each other.
 *   determinism  integer arithmetic and integer atomics that commute (add, min, max) only: the result is a function of the inputs alone,
 *                bit-identical from run to run and independent of scheduling.
 * The contract is that of gg_fuse_states: NO MAP IS READ OR CHANGED -- no layer, position, freshness, configuration, score or liveness flag,
 * and the lazily kept layers stay pending.  n <= n_slots (GG_ERR_CAPACITY): the call takes an entry of the same ring of parameter entries
 * and orders itself on `stream` as that call does; it enqueues and returns.  The caller's device buffers must stay valid and unmodified
 * until `stream` has passed the call.  With min_cells == 1 and no d_cell_size the size and filter launches do not run.
 * Argument errors write nothing and change nothing: GG_ERR_INVALID for null ctx (before the device is touched), null x, n < 0; and with
 * n > 0: null d_seeds or d_cell_cluster, lo > hi, a connectivity that is not 4 or 8, an unknown order, seed_stride or plane_stride
 * < rows * cols, value_stride < rows * cols with d_values, size_stride < rows * cols with d_cell_size, min_cells < 1, min_cells > 1
 * without d_cell_size, max_regions < 0, d_regions given with max_regions == 0 or not 8-byte aligned, overlapping buffers;
 * GG_ERR_CAPACITY for n > n_slots.  n == 0 is GG_OK before anything else is looked at.  The first call of a context may allocate
 * (GG_ERR_NOMEM) and block; later calls only enqueue.  Capture into a caller's graph is not supported. */
typedef struct gg_region {         /* 48 bytes: record k describes kept component k of the map */
    int32_t cells;                 /* cells of the region */
    int32_t row_min, row_max, col_min, col_max;
    int32_t first_cell;            /* smallest linear cell index of the region, in `order` */
    int32_t value_cell;            /* L of the cell that attains value_min, the smallest among equals; -1 without d_values */
    int32_t value_min;             /* the minimum of d_values over the region; INT32_MAX without d_values */
    int64_t sum_row, sum_col;      /* sums of (row, col) over its cells: centroid = sum / cells */
} gg_region;
typedef struct gg_plane_clusters {
    int n;                         /* maps */
    const int32_t *d_seeds;        /* [n] planes, seed_stride apart: a member where lo <= word <= hi; required */
    size_t seed_stride;            /* int32 words, >= rows * cols */
    int32_t lo, hi;                /* lo <= hi */
    int connectivity;              /* 4 or 8 */
    int min_cells;                 /* >= 1: a component of fewer cells is dropped */
    int order;                     /* GG_PLANES_COLMAJOR / GG_PLANES_ROWMAJOR, of every plane of the call */
    const int32_t *d_values;       /* [n] planes, value_stride apart; nullable */
    size_t value_stride;           /* >= rows * cols with d_values */
    int32_t *d_cell_cluster;       /* [n] planes of rows * cols int32, plane_stride apart; required */
    size_t plane_stride;           /* >= rows * cols */
    int32_t *d_cell_size;          /* [n] planes, size_stride apart; nullable when min_cells == 1 */
    size_t size_stride;            /* >= rows * cols with d_cell_size */
    int32_t *d_heads;              /* [n][4]: K, dropped components, member cells, kept cells; nullable */
    gg_region *d_regions;          /* [n][max_regions], 8-byte aligned; nullable */
    int max_regions;               /* >= 0; must be > 0 when d_regions is given */
} gg_plane_clusters;
int gg_cluster_planes(gg_context *ctx, const gg_plane_clusters *x, void *stream);
#define GG_HAS_CLUSTER_PLANES 1

/* insert_cloud's per-point decision (include/groundgrid/GroundSegmentation.h:55): after a filter call,
 * class (GG_CLASS_*) and cell (row + col*rows, -1 outside) of every input point of `slot`. */
int gg_get_point_classes(gg_context *ctx, int slot, size_t n, uint8_t *out_class, int32_t *out_cell);

/* ---- the stage members of the reference's class, one by one (include/groundgrid/GroundSegmentation.h:59-62) --------
 * filter_cloud runs them as stages of one launch sequence; the header also declares them public, so the drop-in library
 * answers a caller that invokes one on its own.  Each runs on the slot's layers AS THEY STAND (whatever the last cloud,
 * gg_set_layer or an earlier stage left) and leaves its results in the slot, synchronously:
 *   GG_STAGE_DETECT_GROUND_PATCHES        detect_ground_patches(map, section), src/GroundSegmentation.cpp:314-340:
 *                                         variance := m2 ./ (points + FLT_MIN) over the whole layer (:323), then
 *                                         detect_ground_patch<3|5> for every cell of quadrant `section` (0: top-left, 1: top-right,
 *                                         2: bottom-left, 3: bottom-right, :325-328; -1: all four, what filter_cloud's four threads do)
 *   GG_STAGE_SPIRAL_GROUND_INTERPOLATION  spiral_ground_interpolation(map, toBase), :398-441, base_z = toBase.transform.translation.z
 *                                         (the only field the function uses, :406-411).  filter_cloud's reset of `points` (:147)
 *                                         is NOT part of it.
 *   GG_STAGE_DETECT_GROUND_PATCH_3 / _5   detect_ground_patch<S>(map, i, j), :343-395 (reads `variance` as it stands)
 *   GG_STAGE_INTERPOLATE_CELL             interpolate_cell(map, x = i, y = j), :445-465
 * The many-cell stages are the kernels of the path (k_patch without the skipping of blocks the last cloud left empty and with
 * the :359 count in Eigen's order, k_sweep); the single-cell ones are one lane of a kernel of their own.  Cell indices whose
 * blocks would leave the map -- UB in the reference -- are GG_ERR_INVALID. */
enum {
    GG_STAGE_DETECT_GROUND_PATCHES = 1,
    GG_STAGE_SPIRAL_GROUND_INTERPOLATION = 2,
    GG_STAGE_DETECT_GROUND_PATCH_3 = 3,
    GG_STAGE_DETECT_GROUND_PATCH_5 = 4,
    GG_STAGE_INTERPOLATE_CELL = 5
};
typedef struct gg_stage_args {
    int section;   /* GG_STAGE_DETECT_GROUND_PATCHES: 0..3, or -1 for all four quadrants */
    int i, j;      /* the single-cell stages: row and column */
    double base_z; /* GG_STAGE_SPIRAL_GROUND_INTERPOLATION */
} gg_stage_args;
int gg_run_stage(gg_context *ctx, int slot, int stage, const gg_stage_args *args);

/* GroundSegmentation::insert_cloud as the member it is (include/groundgrid/GroundSegmentation.h:55, src/GroundSegmentation.cpp:200-311):
 * the points cloud[start, end) against the slot's map AS IT STANDS -- no per-call reset (:61-75 is filter_cloud's): `pointsRaw` and the seven
 * recurrences of :296-309 continue from what the layers hold, a cell's count from wherever an earlier range left it; the outlier test of
 * :243-279 reads ground / groundpatch as they are.  out_class / out_cell (each end - start entries, either may be null) = per point of the
 * range, in cloud order, its GG_CLASS_* and its cell (row + col * rows; -1 outside the map): the three lists the reference appends to
 * are the points of class KEPT (`point_index`, with their cells), IGNORED (`ignored`, with their cells) and OUTLIER (`outliers`), each
 * in cloud order -- the host mirrors build them from these two arrays.  Synchronous; ABI v6. */
int gg_insert_cloud(gg_context *ctx, int slot, const gg_point32 *cloud, size_t start, size_t end, const float origin[3], uint8_t *out_class, int32_t *out_cell);

/* ---- measurement --------------------------------------------------------------------------- */

enum {
    GG_K_CLASSIFY = 0, /* K1: insert_cloud classify + tile key (:219-279)                 */
    GG_K_SCAN = 1,     /*     exclusive scan of tile histograms                            */
    GG_K_SCATTER = 2,  /*     stable scatter into Morton-tile order                        */
    GG_K_REDUCE = 3,   /* K2: ordered per-cell reductions (:282-309) + variance (:323)    */
    GG_K_PATCH = 4,    /* K3: detect_ground_patch<3|5> stencil (:330-395)                 */
    GG_K_SPIRAL = 5,   /* K4: spiral_ground_interpolation (:398-465)                       */
    GG_K_LABEL = 6,    /* K5: label loop (:147-189)                                        */
    GG_NUM_KERNELS = 7
};
/* With GG_FLAG_PROFILE: accumulated milliseconds and launch counts per kernel since the last reset. */
int gg_get_kernel_times(gg_context *ctx, double ms[GG_NUM_KERNELS], int64_t launches[GG_NUM_KERNELS], int reset);
const char *gg_kernel_name(int k);
/* ... and the same for k_score, the evaluator's count behind the label loop of a launch with a scoring slot (GG_NUM_KERNELS and the
 * arrays above keep their size) */
int gg_get_score_kernel_time(gg_context *ctx, double *ms, int64_t *launches, int reset);
int gg_abi_version(void);

/* Testing hook, runs on the host (no GPU): the terrain sweep the device runs (ring-per-lane dataflow, csrc/sweep_core.h) --
 * the same per-lane code -- emulated wavefront by wavefront with a seeded interleaving of the wavefronts (seed 0 = round
 * robin) and, if late_loads, every layer load resolved only when it is used.  gp2 = interleaved (ground, groundpatch)
 * [n*n][2] in Eigen's column-major cell order, updated in place like spiral_ground_interpolation
 * (src/GroundSegmentation.cpp:398-465) would.
 * stats (nullable, 8 longs): wave-steps, stalls, layer loads, stores, LDS operations, LDS bytes, wavefronts, decay radius^2.
 * Returns 0, or -10 if the wavefronts deadlock. */
int gg_debug_emulate_ring_sweep(int n, double resolution, float min_dist_squared, float *gp2, float base_z,
                                double occupied_cells_decrease_factor, unsigned seed, int late_loads, long *stats);
/* Testing hook, host only: the sweep's wait test -- one compare per half step against the last step the progress counters read last
 * cover (csrc/sweep_core.h ChainSync::cover) -- held to the closed-form needs it inverts, for every side, ring group, counter value and
 * wave-step of an n x n map.  Returns the number of disagreements (0), -1 for n < 8. */
long gg_debug_sweep_sync_selftest(int n);

#ifdef __cplusplus
}
#endif
#endif
