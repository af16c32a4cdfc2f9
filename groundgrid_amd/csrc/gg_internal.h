// gg_internal.h -- device/host shared structures of libgroundgrid_hip (gfx950 only).
//
// HBM layout of one context (see DESIGN.md "Data layout"):
//   shared   : expectedPoints[C]  spiral schedule  tile rank tables
//   per slot : the nine per-call layers tile by tile (percall_index below; ground / groundpatch: gp2, gp_layout.h)
//              rec[Nmax]    (z, key)     cloud order     written by K1
//              sorted[Nmax] (z, key)     Morton-tile order, cloud order inside a tile (stable)
//              hist[NCH][T] per-wave-chunk tile histogram -> exclusive offsets after the scan
//              chunk_emit[NCH][4], totals[4], tile_start[T+1]
//              labels[Nmax], out_index[Nmax], pts16[Nmax] (host staging path)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "groundgrid_hip.h"
#include "gp_layout.h"

namespace gg {

constexpr int TILE = 16;             // cells per tile edge (K2 work-group = one tile, one thread per cell)
constexpr int TILE_CELLS = TILE * TILE;
constexpr uint32_t KEY_OUTSIDE = 0xFFFFFFFFu;
constexpr int K2_DBG_WGS = 32768;  // slots of k_reduce's phase counters (GG_K2_DEBUG=9)
// Launch geometry that changes with the batch size -- named here because docs and tests refer to it:
constexpr int PW_BIG_CONTEXT_SLOTS = 128;      // contexts with at least this many slots use 2048-point wave chunks (else 1024)
constexpr int SWEEP_LATENCY_MAX_CLOUDS = 256;  // (= CUs) k_sweep: launches of at most this many work-groups give every 64-ring group of a side
                                               // its own wavefront (up to 3 per side), and clouds are cut into as many work-groups
                                               // ("parts") as keep the launch within it; bigger launches use make_params' throughput setting
constexpr int K2_MIN_GROUPS_PER_CLOUD = 64;    // k_reduce: work-groups per cloud = max(4096 / clouds, this)
constexpr int PACKED_TILE_COUNTERS_MIN_T = 1024; // maps with more tiles keep K1's / k_scatter's per-wavefront tile counters as 16-bit halves
                                                 // (a chunk has fewer than 65536 points): 71 -> 40 KB of LDS per work-group at 3969 tiles
constexpr int K2_LIGHT_MAX = 512; // tiles with at most this many records are reduced by a single wavefront (k2_reduce.hip)
// key = tile_rank << 12 | emit << 10 | class << 8 | cell_in_tile (row_in_tile | col_in_tile << 4)
constexpr int KEY_TILE_SHIFT = 12;
constexpr int SCAN_MAX_PARTS = 16, SCAN_SYNC_WORDS = 1 + SCAN_MAX_PARTS; // (k_sort.hip k_scan_parts)
constexpr uint32_t KEY_EMIT_BIT = 1u << 10;
constexpr int KEY_CLASS_SHIFT = 8;

// device copy of gg_config plus the constants derived from it once per set_config
struct DevConfig {
    int point_count_cell_variance_threshold;
    int max_ring;
    double outlier_tolerance;
    double gpd_min_point_count_threshold;   // ground_patch_detection_minimum_point_count_threshold
    double patch_size_change_distance_sq;   // pow(patch_size_change_distance, 2.0)
    double occupied_cells_decrease_factor;
    double occupied_cells_point_count_factor;
    double occupied_cells_point_count_factor_x2; // factor * (double)2.0f
    double min_outlier_detection_ground_confidence;
    double distance_factor_sq;              // pow(distance_factor, 2.0)
    double minimum_distance_factor_sq;      // pow(minimum_distance_factor, 2.0)
    double minimum_distance_factor_x10_sq;  // pow(minimum_distance_factor*10, 2.0)
    double min_dist_fac;                    // minimum_distance_factor * 5   (:154)
    double min_point_height_thres;          // :155
    double min_point_height_obs_thres;      // :156
    // the sweep's decay (:464, sweep_core.h decayed_confidence): 1 / occupied_cells_decrease_factor and "the product form is safe" (>= 1.25)
    double inv_decrease;
    int decay_fast;
};

struct Geometry {
    int rows, cols;          // grid_map size
    int C;                   // rows * cols
    int tiles_r, tiles_c, T; // tile grid
    double resolution;       // (double)resolution_f
    double inv_resolution;   // 1.0 / resolution (fast path of the index division, gg_device.h)
    double length0, length1; // size * resolution
    double half0, half1;     // 0.5 * length  (getVectorToOrigin)
    float resolution_f;      // (float)map.getResolution()
    float min_dist_squared;
    int center;              // rows/2 - 1
};

// per-cloud parameters of one batched call (device array, one entry per cloud of the batch)
struct CloudParams {
    int slot;
    int n_points;
    float ox, oy, oz;
    float base_z;   // (float)translation.z
    double pos_x, pos_y;
    int has_tf;     // points are in the sensor frame: p_map = (float)(R p + t) first (src/GroundGridNodelet.cpp:166-181)
    int fresh;      // the slot's (ground, confidence) layer holds the reset values by DEFINITION -- only its never-swept border, Arena::gp_fresh_cell
                    // and what k_patch writes in this call (tagged in bit 31 of the confidence word) count; the sweep of this call makes the layer real
    int no_confidence; // the slot's groundpatch layer is known to hold nothing above 0.01 (fresh or only scrolled since
                    // gg_reset_map): the line-of-sight test (:269 needs groundpatch(I) > 0.01f) cannot fire, K1 skips the walks
    double tf[12];  // map <- cloud frame, 3x4 row-major (R | t)
    int label_shift; // bytes added to this cloud's d_labels row (the host call places a cloud's labels right behind its n index entries -- one
                     // download for both -- and a captured launch must not bake that n in: it travels here)
    int io_index;    // the cloud's row of the batch's I/O buffers (d_points, d_labels, ...): its position in gg_batch, which is not its position
                     // in the parameter array when a batch runs as two halves (GG_FLAG_CONCURRENT_HALVES)
    int cfg_index = -1; // the slot has a configuration of its own (gg_set_slot_configs): its entry of Arena::slot_cfg; -1 = the context's (Arena::cfg)
};

// everything a kernel needs to find its data
struct Arena {
    Geometry g;
    DevConfig cfg;
    // shared
    const float *expected;        // [C]
    const float4 *patch_table;    // [C] what detect_ground_patches needs to know about a cell that depends on the geometry and the
                                  // configuration only (rebuilt by gg_set_config, k3_patch.hip PatchCell): x = expectedPoints (:358),
                                  // y = the point-count threshold of :364-365, NEGATIVE when the cell takes 3 x 3 blocks (:334), +inf
                                  // when the quadrant loops never visit it (:325-328); z = varThresholdsq (:369); w = the cell's
                                  // element in the (ground, confidence) layer (an int, gp_layout.h)
    const uint16_t *tile_rank;    // [T] tile (tr + tc*tiles_r) -> Morton rank
    const uint16_t *rank_tile;    // [T] Morton rank -> tile
    const uint32_t *rank_cell0;   // [T] Morton rank -> first row | first col << 16 of the tile (per-point lookups: no division)
    // per slot (slot s at base + s * stride)
    float *layers;  size_t slot_layer_stride;  // the nine per-call layers of slot s, TILE BY TILE (percall_block below): layers + s*slot_layer_stride
    const uint32_t *gp_valid;     // one bit per element of the gp2 order: does gg_reset_maps fill it (the 128-byte lines that hold cells; the rest is padding)
    float2 *gp2;    size_t gp2_stride;    GpLayout gpl;              // (ground, confidence) of slot s: gp2 + s*gp2_stride, element order gp_layout.h
    // FRESH maps (gg_reset_maps did not write the interior: CloudParams::fresh).  The layer's memory is whatever the slot's last use left
    // there -- positive confidences, always: every confidence the path writes is positive (k_patch: min(old + 0.1, 0.5) or a positive average;
    // the sweep: max(w - w / f, 0.001); the reset: 1e-7), and a slot whose memory may hold anything else is filled by its next reset
    // (gg_context::gp_tainted).  On a fresh launch k_patch stores its confidences with bit 31 SET; k_sweep<FRESH> loads the cells the plain
    // kernel loads and takes a cell as it is (confidence |w|) iff the bit is set, else the reset's pair (sweep_core.h sw_untag).  Every cell
    // the sweep visits is stored positive, the tagged cells nobody visits (ring >= c) are cleared when the kernel ends: after a complete call
    // no cell carries the tag, which is why stale memory always reads as "not written in this call".
    // gp_fresh_cell: a padding element that holds the reset values (ground = odom_z, confidence = 1e-7).
    // gp_bits*: a region behind each slot's layer, RESERVED -- it held one written-cell bit per element before the tag; no kernel touches it
    unsigned long long *gp_bits;  size_t gp_bits_stride;  int gp_fresh_cell;
    int gp_bits_off, gp_bits_words;           // (the reserved region: 8-byte element gp_bits_off of the slot's gp2 region, gp_bits = gp2 + that)
    const int *gp_border;  int gp_border_n;   // the elements of the cells no sweep visits (ring >= c): k_sweep<FRESH> writes the reset's pair into the untagged ones
    int gp_border_patched;                    // k_patch's quadrant loops (:325-328) reach a cell of ring >= c (maps with an odd number of rows): border cells can carry the tag
    int fresh_launch;                         // this launch's maps are all fresh (CloudParams::fresh): k_sweep's FRESH variant
    uint2 *rec;     uint2 *sorted;  size_t point_stride;            // per slot Nmax
    float *zcell;   size_t zcell_stride;  // per slot: the KEPT heights grouped by cell (K2's stable cell sort), Nmax + 32 T + 64
    uint32_t *hist;        size_t hist_stride;   // NCH * hist_pitch
    int hist_pitch;        // words per chunk row of `hist`: T rounded up to a multiple of 4 (rows are read and written 16 bytes at a time)
    uint32_t *front_sync;  // [2 n_slots + 16] words the fused front end (k1_classify.hip) synchronises through, zeroed before every launch
                           // that uses them: arrivals per slot, "scanned" flag per slot, 8 ticket counters (one per XCD)
    uint32_t *dev_error;   // one word of host-mapped pinned memory: a kernel that gives up a bounded wait leaves a GG_DEVERR_* code
                           // here and the next gg_* call that synchronises reports GG_ERR_HIP instead of hanging
    uint32_t *chunk_emit;  size_t emit_stride;   // NCH * 4
    uint32_t *totals;      // [slot][4]  (emitted kept, emitted ignored, outliers, in-map)
    uint32_t *tile_start;  size_t tile_start_stride; // T + 1
    uint32_t *tile_live;   size_t tile_live_stride;  // [slot][T] by Morton rank: bit k = HALF COLUMN k of the tile (cells 8k .. 8k + 7 of the
                                                     // tile's cell order row + 16 col: 8 cells, one 32-byte sector per layer) physically
                                                     // HOLDS its values in the nine per-call layers.  A half column whose bit is clear
                                                     // holds stale bytes and logically has the per-call reset values (:61-75) -- the
                                                     // per-call layers are stored SPARSELY: K2 writes (and marks) exactly the half columns
                                                     // that hold an in-map record of this cloud, k_scan clears the masks of tiles without
                                                     // records, and every reader (K3's staging, gg_get_layer, the image kernels)
                                                     // substitutes the reset values through cell_is_live().  Nothing ever has to "clean"
                                                     // the cells a previous cloud left behind.  (Half columns: a scan line crosses a
                                                     // tile as an arc that touches most columns in one or two cells -- 27 % fewer layer
                                                     // bytes than with whole columns on a street scene.)
    uint4 *tile_list;      size_t tile_list_stride;  // [slot][T] K2's work lists (k_scan): light tiles from the front, dense tiles from the back; an
                                                     // entry is everything K2 needs to know about the tile without another dependent
                                                     // lookup: x = Morton rank, y / z = first / end
                                                     // of its records in `sorted`, w = first row | first col << 16
    uint32_t *tile_list_cnt;                         // [slot][2] number of light / dense tiles
    unsigned long long *scan_sync; // [n_slots][SCAN_SYNC_WORDS] k_scan as several work-groups per cloud (sort_core.h "PARTS"): ticket counter, then one
                                   // word per part; zeroed before every such launch
    uint32_t *front_sync2, *sweep_sync2; // the same two regions once more, for the half of a batch that runs on the library's side stream
    unsigned long long *scan_sync2;      // ... and the scan's (its own region: consecutive divided batches need not have equal halves)
    uint32_t *sweep_sync; // [4] ticket counter, finished work-groups, epoch of k_sweep launches with several work-groups per cloud (k4_sweep.hip)
    unsigned long long *sweep_xchg; size_t sweep_xchg_stride; // [slot] exchange region between the work-groups of one sweep (sweep_core.h "Parts"), in 64-bit words
    float *sweep_rec; size_t sweep_rec_stride; int sweep_rec_clouds; // scratch of the pair sweep (k4p_sweep_pair.hip): the records of up to
                                                                     // sweep_rec_clouds clouds of ONE launch (cloud b of the launch at sweep_rec + b * stride floats)
    unsigned long long *pair_dbg; // tools (GG_PAIR_TIMING=1 at gg_create): cycle counters of the pair sweep's wavefronts, cloud 0 of a launch; else nullptr
    int n_slots; // independent map states of the context
    int PW;    // points per wave-chunk
    int NCH;   // chunks per cloud (capacity)
    // launch geometry overrides (0 = the launchers' defaults).  Set at gg_create from the environment (GG_SWEEP_WAVES,
    // GG_K2_PER_CLOUD, GG_K2_DENSE_SHARE; GG_PW above) or per context by gg_debug_set_tuning: tools measure with them, and the
    // parity tests force every geometry the launchers can pick (tests/test_gpu_parity.py) at small batch sizes.
    int tune_sweep_waves;   // chain wavefronts per side of k_sweep
    int tune_sweep_gpw;     // ring groups per work-group of k_sweep (sweep_core.h "Parts"); default min(groups, 3)
    int tune_sweep_split;   // k_sweep "split steps": 0 = when a launch has one ring group per work-group and at most 256 work-groups, 1 = whenever gpw == 1, 2 = never
    int tune_sweep_pair;    // the pair sweeps: 0 = sweep_pair.h for launches of at most sweep_rec_clouds clouds, k_sweep for larger ones; 2 = never (k_sweep
                            // always); 4 = sweep_pairb.h (the pair sweep on the layer in place) for every launch
    int tune_sweep_pair_wgs; // work-groups per cloud of the pair sweep: 0 / 2 = one per pair of sides (two CUs), 1 = both pairs in one
    int tune_sweep_pair_waves; // chain wavefronts per pair (0 = one per 32-ring group, as many as fit)
    int tune_sweep_poll_cap; // tests: polls after which k_sweep's waits give up (0 = about a second)
    int tune_sweep_fault;   // tests: sweep::Params::debug_fault
    int tune_scan_fault;    // tests: 1 = the first part of a cloud's scan never publishes its sums (the waits of the others run out: GG_DEVERR_SCAN_WAIT)
    int tune_scan_poll_cap; // tests: polls after which a scan part's wait gives up (0 = sort_core.h SCAN_WAIT_POLLS, several seconds)
    int tune_scan_parts;    // tests: work-groups per cloud in k_scan (0 = the launcher's choice, k_sort.hip scan_parts)
    int tune_front;         // the front end (classify + tile sort): 0 = the launcher's choice, 1 = three launches (k_classify, k_scan,
                            // k_scatter), 2 = the scan inside k_classify (the last work-group of a cloud to finish scans it), 3 = one launch
                            // (after the scan every work-group scatters its own chunks)
    int tune_k2_per_cloud;  // minimum work-groups per cloud of k_reduce
    int tune_k2_dense_share; // sixteenths of them that walk the dense list
    int k2_skip;             // measurement (GG_K2_SKIP): 1 = k_reduce leaves the light tiles out, 2 = the dense tiles
    unsigned flags;
    int k2_debug;        // env GG_K2_DEBUG (measurement only, libraries built with -DGG_INSTRUMENT: gg_device.h GG_DEBUG_SWITCH): 1 = k_reduce stops after the tile lookup, 2 = after step 1, 3 = after step 3,
                         // 9 = per-phase cycle counters into k2_dbg (tools/k2_phases.py)
    unsigned long long *k2_dbg; // [64] when k2_debug == 9
    int k5_debug;        // env GG_K5_DEBUG (measurement only, results void), bits: 1 = no gathers (every lane reads element 0), 2 = no label / index stores,
                         // 4 = no `points` atomics
    int k3_debug;        // env GG_K3_DEBUG (measurement only): 1 = k_patch stops after the tile check, 2 = after staging, 3 = after the first test (:364)
    int eigen_reduction; // gg_conventions::eigen_reduction (GG_EIGEN_33 / GG_EIGEN_34_SSE): order of the 5x5 block sums in K3
    // per-slot configurations (gg_set_slot_configs): entry s = slot s's own DevConfig, read through CloudParams::cfg_index.  Uploaded when
    // the slot configurations change, never per launch.  slot_cfg_launch: some cloud of THIS launch has one -- the launchers then pick the
    // SLOT_CFG variants of k_classify, k_patch, the sweeps and k_label, which read the configuration per cloud; a launch without one runs
    // the kernels it always ran, with Arena::cfg and Arena::patch_table
    const DevConfig *slot_cfg;
    int slot_cfg_launch;
};

// The nine per-call layers (everything but ground / groundpatch) are stored tile by tile: the 16x16 tile of Morton rank r owns the
// block [r * PERCALL_BLOCK, (r + 1) * PERCALL_BLOCK) of its slot, laid out [layer position][column in tile][row in tile] -- 9 x 256
// floats, 9 KiB, every (layer, column) a 64-byte line segment.  K2 writes a tile's nine layers as ONE contiguous region instead of
// 144 segments 1456 bytes apart in nine planes (measured: k_reduce 1.47 -> 1.31 ms per 1024 clouds with the same bytes), K5
// addresses a point's cell straight from its key (tile rank, cell in tile) without the tile's origin, and K3's block of 8 columns
// is 512 contiguous bytes per layer.  The order of the layers inside a block puts the three K3 reads first and the three that
// GG_FLAG_MINIMAL_LAYERS leaves out last.  The dense column-major matrices of the reference exist at the host boundary only
// (gg_get_layer / gg_set_layer, k6_wire.hip).
constexpr int PERCALL_LAYERS = 9;
constexpr int PERCALL_BLOCK = PERCALL_LAYERS * TILE * TILE;
enum : int { PL_POINTS = 0, PL_VARIANCE = 1, PL_MINGROUNDHEIGHT = 2, PL_M2 = 3, PL_POINTSRAW = 4, PL_MEANVARIANCE = 5, PL_MAXGROUNDHEIGHT = 6,
             PL_GROUNDCANDIDATES = 7, PL_PLANEDIST = 8 };
__host__ __device__ inline int percall_position(int layer) // gg_layer -> position in a block (-1: ground / groundpatch live elsewhere)
{
    switch (layer) {
    case GG_LAYER_POINTS: return PL_POINTS;
    case GG_LAYER_VARIANCE: return PL_VARIANCE;
    case GG_LAYER_MINGROUNDHEIGHT: return PL_MINGROUNDHEIGHT;
    case GG_LAYER_M2: return PL_M2;
    case GG_LAYER_POINTSRAW: return PL_POINTSRAW;
    case GG_LAYER_MEANVARIANCE: return PL_MEANVARIANCE;
    case GG_LAYER_MAXGROUNDHEIGHT: return PL_MAXGROUNDHEIGHT;
    case GG_LAYER_GROUNDCANDIDATES: return PL_GROUNDCANDIDATES;
    case GG_LAYER_PLANEDIST: return PL_PLANEDIST;
    default: return -1;
    }
}
__host__ __device__ inline float *percall_ptr(const Arena &a, int slot) { return a.layers + (size_t)slot * a.slot_layer_stride; }
// element of (tile rank, layer position, cell in tile = row in tile + 16 * column in tile)
__host__ __device__ inline size_t percall_index(int rank, int position, int cell) { return (size_t)rank * PERCALL_BLOCK + (size_t)position * (TILE * TILE) + (size_t)cell; }
// ... of map cell (row, col)
__device__ inline size_t percall_index_of(const Arena &a, int position, int row, int col)
{
    return percall_index(a.tile_rank[(row / TILE) + (col / TILE) * a.g.tiles_r], position, (row % TILE) + (col % TILE) * TILE);
}

// `ground` and `groundpatch` (confidence) are always used together -- confidence-weighted height -- and are the only
// state that persists from cloud to cloud.  They are stored INTERLEAVED as float2 (x = ground, y = confidence), one 8-byte
// request instead of two 4-byte ones everywhere, in the sheared element order of gp_layout.h (the terrain sweep's
// wavefronts then read and write 512 contiguous bytes per access); the plane slots GG_LAYER_GROUND / GG_LAYER_GROUNDPATCH
// of `layers` are unused.  gg_get_layer / gg_set_layer convert at the host boundary.
// the per-call reset value of a layer (:61-75, :147): what a cell outside the live columns logically holds
__host__ __device__ inline float layer_reset_value(int layer)
{
    return layer == GG_LAYER_MINGROUNDHEIGHT ? 3.402823466e+38f /* FLT_MAX, :72 */ : layer == GG_LAYER_MAXGROUNDHEIGHT ? 1.175494351e-38f /* FLT_MIN (sic), :73 */ : 0.0f;
}
// the bit of tile_live that covers `cell` = row in tile + 16 * column in tile
__host__ __device__ inline int live_bit(int cell) { return cell >> 3; }
// does cell (row, col) of `slot` physically hold its per-call layer values (Arena::tile_live)?
__device__ inline bool cell_is_live(const Arena &a, int slot, int row, int col)
{
    const int rank = a.tile_rank[(row / TILE) + (col / TILE) * a.g.tiles_r];
    return ((a.tile_live[(size_t)slot * a.tile_live_stride + rank] >> live_bit((row % TILE) + (col % TILE) * TILE)) & 1u) != 0u;
}

__host__ __device__ inline float2 *gp2_ptr(const Arena &a, int slot) { return a.gp2 + (size_t)slot * a.gp2_stride; }
__host__ __device__ inline int gp_idx(const Arena &a, int row, int col) { return gp_index(a.gpl, row, col); }

// I/O pointers of one batched call
struct BatchIO {
    const void *d_points;
    size_t cloud_stride;
    int point_format;
    uint8_t *d_labels;
    int32_t *d_out_index;
    gg_point32 *d_out_clouds;
    int32_t *d_out_counts;
    uint8_t *d_label_masks;
    uint8_t *d_out_pc2;
};

// The evaluator counters (gg_set_slot_scoring, k8_score.hip).  Kept out of Arena and CloudParams: the kernels of a launch that does not
// score take the arguments they always took.  A slot's counters have the layout of gg_slot_scores: clouds, then [bin][non-ground, ground]
constexpr int SCORE_BINS = GG_SCORE_MAX_LABELS + 1;  // the listed ids, then "every other id"
constexpr int SCORE_WORDS = 1 + SCORE_BINS * 2;      // 64-bit words per slot
struct ScoreArgs {
    const uint8_t *ring_bin;      // [65536] ring -> bin (gg_set_score_labels)
    const uint8_t *slot_on;       // [n_slots] does the slot score
    unsigned long long *scores;   // [n_slots][SCORE_WORDS]
};

// gg_export_layers (k9_export.hip): one entry per exported map, and what the kernels of a call share.  The export table cuts the map into
// blocks of EXPORT_TILE x EXPORT_TILE cells (block = block row + block column * blocks_r) and lists every block's cells sorted by their
// element in the sheared (ground, confidence) layer: block b owns entries [block_off[b], block_off[b + 1]) of `elem` (the element) and
// `cell` (row in block | column in block << 6)
constexpr int EXPORT_TILE = 64;
struct ExportMap {
    int slot;
    int fresh;     // the map is fresh (gg_context::fresh): ground = fresh_z, groundpatch = 1e-7 everywhere, its layer is not read
    float fresh_z;
    int reserved;
};
// gg_export_layers and gg_import_layers (k10_import.hip) share the map entries, the table and the addressing: one record, whose `planes` the
// export writes and the import only reads
struct PlaneArgs {
    const ExportMap *maps;
    const uint32_t *block_off, *elem;
    const uint16_t *cell;
    int blocks_r, blocks_c;
    unsigned mask; // bit per gg_layer (launch_slopes: per GG_SLOPE_*)
    int n_planes;  // its popcount
    int order;     // GG_PLANES_*
    float *planes; // map i's plane k (the k-th layer of `mask` in gg_layer order) at planes + (i * n_planes + k) * plane_stride
    size_t plane_stride;
};

// gg_export_images (k11_images.hip): the u8 layer images and the terrain images of the listed maps.  The same map entries and table as
// PlaneArgs.  The bounds of a (map, layer) reach the image launch as `n_parts` partial (min, max) pairs the bounds launch wrote:
// partials[((map * n_planes + k) * n_parts + part) * 2]; a part without a finite cell holds (+inf, -inf).
constexpr int IMAGE_GATHER_PARTS = 64; // work-groups per map of the cell-by-cell form (variant 1) = its partial pairs per plane
struct ImageArgs {
    const ExportMap *maps;
    const uint32_t *block_off, *elem;
    const uint16_t *cell;
    int blocks_r, blocks_c;
    unsigned mask;        // the u8 images: bit per gg_layer (0: none)
    int n_planes;         // its popcount
    uint8_t *images;      // map i's image k at images + (i * n_planes + k) * image_stride, rows x cols row-major bytes
    size_t image_stride;  // bytes
    float *partials;      // call scratch (above)
    int n_parts;
    float *bounds;        // [map][n_planes][2] lower, upper; null: nobody asked
    float *terrain;       // map i at terrain + i * terrain_stride; null: no terrain image
    size_t terrain_stride; // floats
    int terrain_layout;   // GG_TERRAIN_*
};
inline int image_parts(const Geometry &g, int variant) // partial pairs per plane of a call
{
    const int blocks = ((g.rows + EXPORT_TILE - 1) / EXPORT_TILE) * ((g.cols + EXPORT_TILE - 1) / EXPORT_TILE);
    const int gather = (g.C + 255) / 256 < IMAGE_GATHER_PARTS ? (g.C + 255) / 256 : IMAGE_GATHER_PARTS;
    return variant == 1 ? gather : blocks;
}

// gg_split_clouds (k12_split.hip): one entry per cloud of a call (a pinned ring entry, like ExportMap), and what its two launches share
struct SplitCloud {
    int slot;
    int n_points;
    int fresh;       // the map is fresh (gg_context::fresh): the ground under every point is fresh_z, its layer is not read
    float fresh_z;
    int has_tf;      // the points are in the sensor frame: p_map = transform_point(tf, p) first
    int io_index;    // the cloud's row of the caller's buffers and of the call's chunk counters: its position in gg_cloud_split
    float ox, oy;    // gg_visibility_clouds: the sensor in the map frame (zero in every other call)
    double pos_x, pos_y; // the map's position when the call was made
    double tf[12];
};
struct SplitSet {
    gg_point16 *points;
    float *height;
    int32_t *source;
};
// the labelled clouds of a call, the first member of every labelled-cloud call's arguments (cloud_walk.h walks them): labelled_clouds_begin fills it
struct CloudArgs {
    const SplitCloud *clouds;
    int point_format;
    const void *points;
    size_t cloud_stride;
    const uint8_t *labels, *masks; // exactly one of the two
    int nch;                       // chunks per cloud of this call: ceil(max n_points / PW), at least 1
};
struct SplitArgs {
    CloudArgs cl;
    SplitSet set[2];               // ground, nonground
    int32_t *counts;               // [cloud][2]
    uint2 *chunk_counts;           // call scratch: [cloud][nch] (points in ground, in nonground) of the chunk, written by k_split_count
};

// gg_rasterize_clouds (k13_raster.hip): what its three launches share.  The per-cloud records are gg_split_clouds' (SplitCloud, the same ring)
struct RasterArgs {
    CloudArgs cl;
    unsigned channel_mask;         // bit per GG_RASTER_*
    int n_planes;                  // its popcount
    int plane_of[GG_NUM_RASTER_CHANNELS]; // channel -> its plane among a cloud's n_planes (-1: not named)
    int order;                     // GG_PLANES_*
    uint32_t *planes;              // the caller's d_dst as 32-bit words: cloud i's plane k at planes + (i * n_planes + k) * plane_stride
    size_t plane_stride;
};

// gg_cluster_clouds (k15_cluster.hip): what its launches share.  The per-cloud records are gg_split_clouds' (SplitCloud, the same ring)
constexpr int CLUSTER_CHUNK_CELLS = 256; // cells per work-group of the cell launches = per root counter of the call scratch
struct ClusterArgs {
    CloudArgs cl;
    int min_points;
    float min_height, max_height;
    int connectivity;              // 4 or 8
    int order;                     // GG_PLANES_*
    uint32_t *planes;              // the caller's d_cell_cluster as 32-bit words: cloud i's plane at planes + i * plane_stride
    size_t plane_stride;
    int32_t *point_cluster;        // [cloud][cloud_stride]; null: nobody asked
    int32_t *n_clusters;           // [cloud]
    uint32_t *records;             // the caller's d_clusters as 32-bit words, eight per gg_cluster: [cloud][max_clusters]; null: no table
    int max_clusters;
    uint32_t *chunk_counts;        // call scratch: [cloud][cell_chunks] roots of the chunk (k_cluster_flatten), then their exclusive prefix (k_cluster_scan)
    int cell_chunks;               // ceil(rows * cols / CLUSTER_CHUNK_CELLS)
};

// gg_clearance_clouds (k16_clearance.hip): what its launches share.  Map i of the call is row i of every buffer.  Cloud mode: `occ` is a
// ClusterArgs on the d_dist2 planes (launch_cluster_occupancy leaves the occupancy there and the first pass reads it in place: seeds ==
// dist2, seed_stride == plane_stride); seed mode: `occ` is not looked at
struct ClearanceArgs {
    ClusterArgs occ;
    bool from_clouds;
    const int32_t *seeds;          // map i's occupancy plane at seeds + i * seed_stride: occupied where the word is >= 0
    size_t seed_stride;
    int order;                     // GG_PLANES_*
    int reach;                     // how far along a row the second pass looks: max_cells, or cols when that is 0 or larger
    uint32_t reach2;               // a dist2 above this is "no obstacle": max_cells squared, or GG_CLEARANCE_NONE - 1
    int32_t *dist2;                // the caller's planes, map i's at + i * plane_stride; dist2 is the working memory
    int32_t *nearest;              // nullable
    float *distance;               // nullable
    size_t plane_stride;
    int32_t *n_occupied;           // [map], nullable
};

// gg_visibility_clouds (k17_visibility.hip): what its launches share.  `occ` is a ClusterArgs on the d_state planes (launch_cluster_occupancy
// leaves the occupancy there); the per-cloud records are gg_split_clouds' with the sensor in (ox, oy)
constexpr size_t VISIBILITY_LDS_MAX = 160 * 1024 - 256;              // bytes of the crossed-cell bitmap one work-group may hold
constexpr size_t VISIBILITY_MAX_CELLS = VISIBILITY_LDS_MAX * 8;      // ... so rows * cols may not exceed this (a side of 1143)
struct VisibilityArgs {
    ClusterArgs occ;
    int order;                     // GG_PLANES_*
    int max_cells;                 // 0: unbounded; R > 0: a ray crosses at most its first R cells
    uint32_t *state;               // the caller's d_state as 32-bit words, cloud i's plane at state + i * plane_stride; the working memory
    size_t plane_stride;
    int32_t *counts;               // [cloud][3] free, unknown, occupied; nullable
    int bitmap_words;              // ceil(rows * cols / 32): 32-bit words of dynamic LDS of the trace launch
};

// gg_fuse_states (k18_fuse.hip): what its one launch takes.  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx`
// contiguous words: (nx, ny) = (cols, rows) row-major, (rows, cols) column-major, and a map's shift arrives as (along x, along y), clamped to
// [-nx, nx] x [-ny, ny].  A work-group owns FUSE_TILE_X x FUSE_TILE_Y cells (_lib.py mirrors the two for the tests of the tile seams)
constexpr int FUSE_TILE_X = 62; // cells along a line: a wavefront minus the one-cell halo on either side
constexpr int FUSE_TILE_Y = 26; // lines
struct FuseArgs {
    const int32_t *state;          // map i's observation plane at state + i * state_stride
    size_t state_stride;
    const int32_t *evidence_in;    // nullable: every prior is 0
    const int2 *shifts;            // device [map] (the call's ring entry); null: all (0, 0)
    int hit, miss, decay, e_min, e_max, free_threshold, occ_threshold;
    int nx, ny, tiles_x;           // tiles_x = ceil(nx / FUSE_TILE_X)
    int32_t *evidence_out;         // map i's planes at + i * plane_stride
    int32_t *fused, *frontier;     // nullable
    size_t plane_stride;
    int32_t *counts;               // [map][4] free, unknown, occupied, frontier; nullable
};

// gg_route_planes (k19_route.hip): what its launches share.  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx`
// contiguous words: (nx, ny) = (cols, rows) row-major, (rows, cols) column-major.  One work-group relaxes a map tile by tile, ROUTE_TILE x
// ROUTE_TILE cells at a time (_lib.py mirrors it for the tests of the tile seams), with one byte per tile in LDS
constexpr int ROUTE_TILE = 64;
constexpr int ROUTE_MAX_TILES = 4096; // tiles of a map (a side of 4096): more is GG_ERR_GEOMETRY
struct RouteArgs {
    const int32_t *blocked;        // map i's plane at blocked + i * blocked_stride: blocked where the word is >= 0; nullable
    size_t blocked_stride;
    const int32_t *cost;           // ... at cost + i * cost_stride: w = min(max(word, 1), cost_max); nullable: w = 1
    size_t cost_stride;
    const int32_t *goals;          // ... at goals + i * goal_stride: a goal where the word is >= 0 and the cell is not blocked
    size_t goal_stride;
    int nx, ny, tiles_x, tiles_y;  // tiles_x = ceil(nx / ROUTE_TILE), tiles_y = ceil(ny / ROUTE_TILE)
    bool row_major;                // a line is a row: what the direction order of d_next, in (row, col) terms, needs to know
    bool diagonals;                // connectivity 8
    uint32_t straight, diagonal;   // step weights
    int cost_max;
    uint32_t reach;                // a tentative D above this is not stored: max_cost, or GG_ROUTE_NONE - 1
    int32_t *dist, *next;          // map i's planes at + i * plane_stride; dist is the working memory, next is nullable
    size_t plane_stride;
    int32_t *counts;               // [map][3] goals, reached, unblocked; nullable
    const int32_t *starts;         // device [map] (the call's ring entry): linear index of the start cell or -1; null: no paths
    int32_t *paths;                // [map][max_path]
    int max_path;
    int32_t *path_len;             // [map]
};

// gg_match_planes (k20_match.hip): what its two launches share.  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx`
// contiguous words: (nx, ny) = (cols, rows) row-major, (rows, cols) column-major.  The rotation, the tie rule and the score volume are in
// (row, col) terms, so the kernel is told the order; shifts and pivots arrive as (row, col), the shifts clamped to [-rows, rows] x [-cols, cols]
constexpr int MATCH_MAX_WINDOW = 32;
constexpr int MATCH_MAX_ROTATIONS = 64;
struct MatchPartial {              // what the work-group of (map, k) leaves for k_match_best
    unsigned long long key;        // S << 32 | ~rank of the best candidate of this k (k20_match.hip match_rank)
    uint32_t ties;                 // candidates of this k whose score equals that S
    uint32_t cells;                // scan cells of the map (the same for every k)
};
struct MatchArgs {
    const int32_t *scan;           // map i's plane at scan + i * scan_stride: a scan cell where the word is > 0
    size_t scan_stride;
    const int32_t *field;          // ... at field + i * field_stride: f = min(max(word, 0), field_max)
    size_t field_stride;
    int field_max;
    const int2 *shifts;            // device [map] (row, col), clamped (the call's ring entry); null: all (0, 0)
    const int2 *pivots;            // device [map] (row, col); null: (rows / 2, cols / 2)
    const int2 *rotations;         // device [K] (cq, sq) in Q14; null: K == 1, (16384, 0)
    int n_rotations;               // K
    int window;                    // W
    int nx, ny;
    bool row_major;
    MatchPartial *partials;        // device [map][K] (the call's ring entry)
    int32_t *best;                 // [map][6]
    int32_t *scores;               // map i's volume at scores + i * score_stride; nullable
    size_t score_stride;
};

// gg_footprint_planes (k21_footprint.hip).  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx` contiguous words: (nx, ny) =
// (cols, rows) row-major, (rows, cols) column-major.  The kernel knows lines and positions along a line alone: the entry point hands it the
// span table per LINE offset (the caller's table row-major, its transpose column-major), every row already turned into the two shifts and the
// erosion level the kernel needs (footprint_pack)
constexpr int FOOTPRINT_MAX_HEADINGS = 32;
constexpr int FOOTPRINT_MAX_RADIUS = 32;
constexpr int FOOTPRINT_TILE = 64; // cells along a line, and lines, of a work-group's tile (_lib.py mirrors it for the tests' seams)
constexpr int FOOTPRINT_TABLE = FOOTPRINT_MAX_HEADINGS * (2 * FOOTPRINT_MAX_RADIUS + 1); // words of one call's table
constexpr uint32_t FOOTPRINT_EMPTY = 0xFFFFFFFFu; // an empty row
// a row (lo, hi) of width w = hi - lo + 1 with p = 2^level the largest power of two <= w: "the w cells from x + lo on are free" is bit
// x + lo and bit x + lo + w - p of the line's erosion by p.  Bit 0 of a line's 128-bit word is position x0 - 32: s1 = lo + 32, s2 = s1 + w - p,
// both in [0, 64]
inline uint32_t footprint_pack(int lo, int hi)
{
    if (lo > hi) return FOOTPRINT_EMPTY;
    const int w = hi - lo + 1;
    int level = 0;
    while ((2 << level) <= w) ++level;
    const int s1 = lo + FOOTPRINT_MAX_RADIUS, s2 = s1 + w - (1 << level);
    return (uint32_t)s1 | (uint32_t)s2 << 8 | (uint32_t)level << 16;
}
struct FootprintArgs {
    const int32_t *blocked;        // map i's plane at blocked + i * blocked_stride: blocked where the word is >= 0
    size_t blocked_stride;
    const uint32_t *table;         // device [K][2 R + 1] packed rows per line offset (the call's ring entry)
    int n_headings;                // K
    int radius;                    // R
    int n_levels;                  // erosion levels the table uses: 1 + the largest level of a row (1 when every row is empty)
    int min_fit;
    int outside_free;
    int nx, ny;
    int tiles_x;                   // tiles along a line
    uint32_t *mask;                // nullable; map i's plane at mask + i * mask_stride
    size_t mask_stride;
    int32_t *fit;                  // nullable; ... at fit + i * fit_stride
    size_t fit_stride;
    int32_t *counts;               // nullable; [map][3]
};

// gg_route_headings (k22_headings.hip).  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx` contiguous words: (nx, ny) =
// (cols, rows) row-major, (rows, cols) column-major.  The kernel knows lines and positions along a line alone: the entry point hands it the
// move table in (line, position) offsets (the caller's (da, db) row-major, swapped column-major), one packed word per move (headings_pack),
// and per heading how a wavefront best walks a tile for that heading's moves (headings_walk).  One work-group relaxes a map tile by tile;
// the tile side depends on the number of headings (headings_tile; _lib.py mirrors it for the tests of the tile seams)
constexpr int HEADINGS_MAX = 32;       // headings
constexpr int HEADINGS_MAX_MOVES = 8;  // moves per heading
constexpr int HEADINGS_MAX_STEP = 3;   // cells a move spans along either axis: the halo of a tile
constexpr int HEADINGS_MAX_COST = 32767;
constexpr int HEADINGS_AT_GOAL = 8;    // d_next of a goal state
constexpr int HEADINGS_TABLE = HEADINGS_MAX * HEADINGS_MAX_MOVES; // packed words of one call's table
constexpr int HEADINGS_MAX_TILES = 4096; // tiles of a map: more is GG_ERR_GEOMETRY
constexpr int HEADINGS_THREADS = 512;  // of the relaxing work-group
inline int headings_tile(int n_headings) { return n_headings <= 16 ? 32 : 16; }
// bits 0-2: line offset + 3, 3-5: position offset + 3, 6-10: k2, 11-25: s; an absent move is the word 0 (s == 0)
inline uint32_t headings_pack(int d_line, int d_pos, int k2, int s)
{
    return s == 0 ? 0u : (uint32_t)(d_line + HEADINGS_MAX_STEP) | (uint32_t)(d_pos + HEADINGS_MAX_STEP) << 3 | (uint32_t)k2 << 6 | (uint32_t)s << 11;
}
// how the slots of k_headings_relax walk a tile for heading k: bit 0: a lane per LINE, stepping along the positions (else a lane per position,
// stepping over the lines); bit 1: from the last step to the first; bit 2: turn the direction round every other sweep; bit 3: swap the axis
// every other pair of sweeps
enum : uint8_t { HEADINGS_WALK_POSITIONS = 1, HEADINGS_WALK_BACK = 2, HEADINGS_WALK_ALT_DIR = 4, HEADINGS_WALK_ALT_AXIS = 8 };
struct HeadingsArgs {
    const uint32_t *mask;          // map i's plane at mask + i * mask_stride: state (k, q) is admissible where bit k of q's word is set
    size_t mask_stride;
    const int32_t *cost;           // ... at cost + i * cost_stride: w = min(max(word, 1), cost_max); nullable: w = 1
    size_t cost_stride;
    const int32_t *goals;          // ... at goals + i * goal_stride: a goal cell where the word is >= 0
    size_t goal_stride;
    uint32_t goal_headings;        // bit k: heading k of a goal cell is a goal state
    int n_headings;                // K
    const uint32_t *table;         // device [K][8] packed moves (the call's ring entry)
    uint8_t walk[HEADINGS_MAX];    // HEADINGS_WALK_* per heading
    int nx, ny, tile, tiles_x, tiles_y;
    int cost_max;
    uint32_t reach;                // a tentative D above this is not stored: max_cost, or GG_ROUTE_NONE - 1
    int max_rounds, max_sweeps;    // min(K * rows * cols, 2^31 - 2) and K * tile * tile: the bounds of the two loops of k_headings_relax
    int32_t *dist;                 // plane k of map i at dist + i * dist_stride + k * plane_stride: the working memory
    size_t dist_stride, plane_stride;
    int32_t *next;                 // nullable; ... at next + i * next_stride + k * next_plane_stride
    size_t next_stride, next_plane_stride;
    int32_t *best, *best_heading;  // nullable; map i's plane at + i * best_stride / best_heading_stride
    size_t best_stride, best_heading_stride;
    int32_t *counts;               // [map][3] goal, reached, admissible states; nullable
    const int2 *starts;            // device [map] (the call's ring entry): (linear index of the start cell or -1, heading); null: no paths
    int32_t *paths;                // map i's row of (cell, heading) pairs at paths + i * path_stride
    size_t path_stride;
    int max_len;                   // pairs of a row
    int32_t *path_len;             // [map]
};

// gg_track_clusters (k23_tracks.hip): what its one launch takes.  Map i of the call is row i of every buffer.  A plane is `ny` lines of `nx`
// contiguous words and the kernel works on (x along a line, y across): row-major x = col, column-major x = row; the gate is a square, so
// only the shift's components and the two coordinate sums follow the order.  `shifts` holds (sx, sy), clamped to [-nx, nx] x [-ny, ny].
constexpr int TRACK_THREADS = 1024;          // one work-group per map; thread c speaks for cluster c in the per-cluster steps
constexpr int TRACK_SLAB_WORDS = 28 * 1024;  // the most words of the contingency matrix a work-group holds at a time (112 KiB)
constexpr int TRACK_FIXED_WORDS = 9;         // LDS words per cluster beside the slab (track_lds_bytes)
constexpr int TRACK_MISC_WORDS = 64;
static_assert(TRACK_THREADS >= GG_TRACK_MAX_CLUSTERS, "one thread per cluster");
static_assert(TRACK_SLAB_WORDS >= GG_TRACK_MAX_CLUSTERS, "a slab holds at least one row");
struct TrackArgs {
    const int32_t *cells;          // this scan's id planes
    size_t cells_stride;
    const int32_t *prev;           // the previous scan's; nullable: no prior (then tracks_in and heads_in are not read)
    size_t prev_stride;
    const gg_track *tracks_in;     // [map][M]
    const int32_t *heads_in;       // [map][4]
    const int2 *shifts;            // device [map] (the call's ring entry); nullable: (0, 0)
    int nx, ny;
    int row_major;                 // sum_row is the sum over y (else over x)
    int M, gate;
    int slab_words;                // min(M * M, TRACK_SLAB_WORDS)
    gg_track *tracks_out;          // [map][M]
    int32_t *heads_out;            // [map][4]
    int32_t *cell_track;           // nullable
    size_t track_stride;
};
inline size_t track_lds_bytes(int M, int slab_words) { return sizeof(uint32_t) * ((size_t)TRACK_FIXED_WORDS * M + TRACK_MISC_WORDS + slab_words); }

// gg_box_clusters (k24_boxes.hip): what its one launch takes.  The per-cloud records are gg_split_clouds' (SplitCloud, the same ring; the call
// has no labels: cl.labels holds the ids' address as a stand-in that the kernel never reads, cl.masks is null).  A work-group holds `slab` clusters at a time: per (cluster, heading) one 64-bit sum and
// four int32 extrema, per cluster one point count.
constexpr int BOX_THREADS = 1024;             // one work-group per cloud
constexpr int BOX_LDS_BUDGET = 144 * 1024;    // the most bytes of a slab
constexpr int BOX_PAIR_BYTES = 24;            // LDS bytes per (cluster, heading)
constexpr int BOX_MAX_SIDE = 4096;            // rows and cols the entry point admits (GG_ERR_GEOMETRY beyond): |u| <= 8 * side + 1
static_assert((8LL * BOX_MAX_SIDE + 1) * 2 * GG_MATCH_UNIT < (1LL << 31), "a = ux * cq + uy * sq and b = uy * cq - ux * sq fit an int32");
// (groundgrid_amd/_lib.py restates BOX_LDS_BUDGET and box_slab_clusters for the tests and tools/bench_boxes.py, which place their cluster
// counts by them: a change of the budget, of BOX_PAIR_BYTES or of the 4 bytes per cluster is made there too; tests/test_box_clusters_cpu.py
// holds the two constants to this text)
struct BoxArgs {
    CloudArgs cl;
    const int32_t *point_cluster;  // [cloud][cloud_stride]
    const int32_t *n_clusters;     // [cloud]
    int K, criterion, M;
    int slab;                      // box_slab_clusters(K, M)
    double scale;                  // GG_BOX_UNIT / resolution
    int32_t rot[2 * GG_BOX_MAX_HEADINGS]; // (cq, sq) of heading k at rot[2 k], rot[2 k + 1]
    gg_box *boxes;                 // [cloud][M]
    unsigned long long *costs;     // [cloud][M][K]; nullable
};
inline int box_slab_clusters(int K, int M) { const int most = BOX_LDS_BUDGET / (BOX_PAIR_BYTES * K + 4); return M < most ? M : most; }
inline size_t box_lds_bytes(int K, int slab) { return ((size_t)BOX_PAIR_BYTES * K + 4) * (size_t)slab + 8 * (size_t)K + 8; } // (+ the rotation table)
static_assert(BOX_LDS_BUDGET / (BOX_PAIR_BYTES * GG_BOX_MAX_HEADINGS + 4) >= 1, "a slab holds at least one cluster");

// gg_score_rollouts (k25_rollouts.hip): what its one launch takes.  Map i of the call is row i of every buffer.  The kernel works in
// (row, col) and forms a cell's linear index by `row_major` alone; the starts arrive checked, three words per map.
constexpr int ROLLOUT_THREADS = 1024;          // one work-group per map; thread t walks rollouts t, t + 1024, ...
struct RolloutArgs {
    const uint32_t *mask;          // map i's plane at mask + i * mask_stride: pose (k, q) is admissible where bit k of q's word is set
    size_t mask_stride;
    const int32_t *cost;           // ... at cost + i * cost_stride: w = min(max(word, 1), cost_max); nullable: w = 1
    size_t cost_stride;
    const int32_t *dist;           // plane k of map i at dist + i * dist_stride + k * plane_stride (gg_route_headings' D); nullable: togo = 0
    size_t dist_stride, plane_stride;
    const int32_t *clear;          // ... at clear + i * clear_stride: squared distances; nullable
    size_t clear_stride;
    const int32_t *table;          // entry (t, p) of map i at table + i * table_stride + (t * P + p) * 4; table_stride == 0: one table
    size_t table_stride;
    const int32_t *starts;         // device [map][3] (the call's ring entry): (r16, c16, k0); r16 == -1: no start
    const int2 *rotations;         // device [K] (the call's ring entry): (cq, sq); null in the absolute frame
    int rows, cols, row_major;
    int K, P, T, frame, reach, cost_max;
    int32_t *records;              // record p of map i at records + i * record_stride + 8 * p
    size_t record_stride;
    int32_t *best;                 // [map][4]; nullable
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device setting: the launchers that need more than 64 KiB of dynamic
// LDS opt in once per DEVICE (a process may hold contexts on several GPUs).  `opt_in` runs under a lock and the device is marked
// only after it returned, so a second thread launching on the same device either sees the mark (the attribute is set) or waits for
// the lock; devices beyond the 64 the mask has bits for opt in on every launch (idempotent).
struct PerDeviceOnce {
    std::atomic<uint64_t> done{0};
    std::mutex lock;
    template <class F> void run(F opt_in)
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const bool tracked = dev >= 0 && dev < 64;
        const uint64_t bit = tracked ? 1ull << dev : 0ull;
        if (tracked && (done.load(std::memory_order_acquire) & bit)) return;
        std::lock_guard<std::mutex> g(lock);
        if (tracked && (done.load(std::memory_order_relaxed) & bit)) return;
        opt_in();
        if (tracked) done.fetch_or(bit, std::memory_order_release);
    }
};

// codes a kernel leaves in Arena::dev_error when it gives up a bounded wait
enum : uint32_t { GG_DEVERR_NONE = 0, GG_DEVERR_FRONT_WAIT = 1 /* k_classify: a cloud's scan never completed */, GG_DEVERR_SWEEP_WAIT = 2 /* k_sweep: a hand-over never arrived */,
                  GG_DEVERR_SCAN_WAIT = 3 /* k_scan in parts: an earlier part's sums never arrived */ };
// the front end's launch shapes (Arena::tune_front)
enum : int { FRONT_AUTO = 0, FRONT_THREE_LAUNCHES = 1, FRONT_SCAN_IN_CLASSIFY = 2, FRONT_ONE_LAUNCH = 3 };
constexpr int FRONT_DEFAULT_SHAPE = FRONT_THREE_LAUNCHES;

// kernel launchers (one per .hip file)
int launch_classify(const Arena &a, const CloudParams *d_params, const BatchIO &io, int n_clouds, int max_n, hipStream_t s); // returns the FRONT_* shape it
                                                                                                                               // ran: the caller adds launch_scan / launch_scatter for what is left
void launch_scan(const Arena &a, const CloudParams *d_params, int n_clouds, hipStream_t s);
void launch_scatter(const Arena &a, const CloudParams *d_params, int n_clouds, int max_n, hipStream_t s);
void launch_reduce(const Arena &a, const CloudParams *d_params, int n_clouds, hipStream_t s);
void launch_stage_insert(const Arena &a, const CloudParams *d_params, hipStream_t s); // gg_insert_cloud: :282-309 continued from the layers as they stand (one slot, dense layers)
void launch_reduce_lazy(const Arena &a, const CloudParams &cp, hipStream_t s); // (GG_FLAG_MINIMAL_LAYERS: the other three layers, one slot)
void launch_reduce_lazy_batch(const Arena &a, const CloudParams *d_params, int n_clouds, hipStream_t s); // (... of n slots in one launch: gg_export_layers)
void launch_export(const Arena &a, const PlaneArgs &x, int n_maps, int variant, hipStream_t s); // k9_export.hip; variant 0 = k_export_tiled, 1 = launch_planes_gather
void launch_import(const Arena &a, const PlaneArgs &x, int n_maps, int variant, hipStream_t s); // k10_import.hip; variant 0 = k_import_tiled, 1 = launch_planes_scatter
void launch_slopes(const Arena &a, const PlaneArgs &x, int n_maps, int variant, hipStream_t s); // k14_slopes.hip; x.mask: bit per GG_SLOPE_*; variant 0 = k_slopes_tiled, 1 = k_slopes_gather (cell by cell)
void launch_images(const Arena &a, const ImageArgs &x, int n_maps, int variant, hipStream_t s);  // k11_images.hip; variant 0 = the tiled kernels, 1 = cell by cell
void launch_split(const Arena &a, const SplitArgs &x, int n_clouds, hipStream_t s);              // k12_split.hip: k_split_count, then k_split_scatter
void launch_raster(const Arena &a, const RasterArgs &x, int n_clouds, hipStream_t s);            // k13_raster.hip: k_raster_planes<false>, k_raster_scatter, k_raster_planes<true>
void launch_cluster(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s);          // k15_cluster.hip: count, seed, merge, flatten, scan, rank, apply, points, finalise
void launch_cluster_occupancy(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s); // k15_cluster.hip: its first three launches alone: x.planes[L] := occupied ? L : 0xFFFFFFFF
void launch_clearance(const Arena &a, const ClearanceArgs &x, int n_maps, hipStream_t s);        // k16_clearance.hip: (occupancy,) columns, rows
void launch_visibility(const Arena &a, const VisibilityArgs &x, int n_clouds, hipStream_t s);    // k17_visibility.hip: occupancy, hits, trace, states
void launch_fuse(const FuseArgs &x, int n_maps, hipStream_t s);                                  // k18_fuse.hip: (counts := 0,) k_fuse_states
void launch_route(const RouteArgs &x, int n_maps, hipStream_t s);                                // k19_route.hip: relax, (counts := 0, next,) (paths)
void launch_match(const MatchArgs &x, int n_maps, hipStream_t s);                                // k20_match.hip: k_match_scores, k_match_best
void launch_footprint(const FootprintArgs &x, int n_maps, hipStream_t s);                        // k21_footprint.hip: (counts := 0,) k_footprint_planes
void launch_headings(const HeadingsArgs &x, int n_maps, hipStream_t s);                          // k22_headings.hip: relax, (counts := 0, next,) (paths)
void launch_tracks(const TrackArgs &x, int n_maps, hipStream_t s);                                // k23_tracks.hip: k_track_clusters
void launch_boxes(const Arena &a, const BoxArgs &x, int n_clouds, hipStream_t s);                 // k24_boxes.hip: k_box_clusters
void launch_rollouts(const RolloutArgs &x, int n_maps, hipStream_t s);                            // k25_rollouts.hip: k_score_rollouts
// the cell-by-cell forms (k6_wire.hip), for any number of maps: every single-map getter and setter is a list of one map (gg_context::d_slot_maps).
// They read x.maps, mask, n_planes, order, planes and plane_stride; the export table is the tiled kernels' alone
void launch_planes_gather(const Arena &a, const PlaneArgs &x, int n_maps, hipStream_t s);   // layers -> dense planes (reset values outside the live half columns)
void launch_planes_scatter(const Arena &a, const PlaneArgs &x, int n_maps, hipStream_t s);  // dense planes -> layers; with a per-call layer named, launch_materialise_maps first
void launch_materialise_maps(const Arena &a, const ExportMap *maps, int n_maps, hipStream_t s); // the reset values into every dead half column of the maps' per-call layers, all marked live
void launch_patch(const Arena &a, const CloudParams *d_params, int n_clouds, hipStream_t s);
void launch_patch_stage(const Arena &a, const CloudParams *d_params, int slot, int section, hipStream_t s); // gg_run_stage: :323 + one quadrant (-1: all) on the slot's layers as they stand
void launch_stage_cell(const Arena &a, int slot, int stage, int i, int j, hipStream_t s);                    // gg_run_stage: detect_ground_patch<S> / interpolate_cell of one cell
namespace sweep {
struct Params;
Params make_params(int n, double resolution, float min_dist_squared, double decrease); // sweep_emul.hip (host)
} // namespace sweep
void launch_sweep(const Arena &a, const sweep::Params &P, const CloudParams *d_params, int n_clouds, hipStream_t s,
                  unsigned long long *dbg = nullptr); // k4_sweep.hip; dbg: 16 x 4 cycle counters of cloud 0's wavefronts (tools)
bool launch_sweep_pair(const Arena &a, const sweep::Params &P, const CloudParams *d_params, int n_clouds, hipStream_t s); // k4p_sweep_pair.hip; false: not this launch
bool sweep_takes_fresh(const Arena &a, const sweep::Params &P, int n_clouds); // k4_sweep.hip: would launch_sweep run k_sweep without split steps (what a launch of fresh maps needs)?
bool launch_sweep_pair_batch(const Arena &a, const sweep::Params &P, const CloudParams *d_params, int n_clouds, hipStream_t s); // k4b_sweep_pair_batch.hip; false: not this launch
size_t sweep_pair_rec_floats(const sweep::Params &P); // scratch floats per cloud of a launch (0: the geometry cannot take the pair sweep)
constexpr int SWEEP_PAIR_MAX_CLOUDS = 16;              // launches of more clouds keep k_sweep
size_t sweep_lds_bytes(const sweep::Params &P);
size_t sweep_xchg_entries(const sweep::Params &P);
void launch_label(const Arena &a, const CloudParams *d_params, const BatchIO &io, int n_clouds, int max_n, hipStream_t s);
void launch_score(const Arena &a, const CloudParams *d_params, const BatchIO &io, const ScoreArgs &sc, int n_clouds, int max_n, hipStream_t s); // k8_score.hip; io.d_label_masks is set
void launch_fill(float *dst, size_t n, float v, hipStream_t s);
void launch_fill_bytes(uint8_t *dst, size_t n, uint8_t v, hipStream_t s);
void launch_fill_strided(float *dst, size_t n, size_t stride, int count, float v, hipStream_t s);   // count regions of n floats, `stride` apart
void launch_fill_percall(const Arena &a, int first_slot, int n_slots, const float init[GG_NUM_LAYERS], hipStream_t s); // every per-call layer of the slots := init[layer]
void launch_fill2_strided(float2 *dst, size_t n, size_t stride, int count, float x, float y, const uint32_t *valid, hipStream_t s);
void launch_fill2(float2 *dst, size_t n, float x, float y, hipStream_t s);
void launch_reset_fresh(const Arena &a, int first_slot, int count, float x, float y, hipStream_t s); // k1_classify.hip k_reset_fresh
void launch_layer_to_u8(const float *layer, int rows, int cols, float *d_bounds, uint8_t *d_img, hipStream_t s);
void launch_terrain_image(const Arena &a, int slot, float *d_img, hipStream_t s);
void launch_scroll(const Arena &a, int slot, float2 *scratch, int s0, int s1, double pos_x, double pos_y, const double plane[4], hipStream_t s);
struct MoveParams; // scroll_core.h
void launch_scroll_batch(const Arena &a, const int2 *cells, const MoveParams *d_params, int n_maps, float2 *scratch, hipStream_t s); // k0b_scroll_batch.hip (gg_move_maps)
void launch_pack16(const gg_point32 *src, gg_point16 *dst, size_t n, hipStream_t s);
void launch_decode_classes(const Arena &a, int slot, size_t n, uint8_t *d_class, int32_t *d_cell, hipStream_t s);

} // namespace gg
