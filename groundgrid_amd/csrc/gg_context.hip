// gg_context.hip -- host side of libgroundgrid_hip.so: the C ABI of include/groundgrid_hip.h.
//
// One gg_context = one device arena (single hipMalloc, sized for n_slots independent map states and
// max_points per cloud), one HIP stream, and the tables GroundSegmentation::init precomputes.
// No CPU fallback: every failure is reported through gg_status / gg_last_error.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>
#include <chrono>

#include <dlfcn.h>
#include <sched.h>
#include <unistd.h>

#include "gg_internal.h"
#include "arena_layout.h"
#include "hip_owned.h"
#include "host_helper.h"
#include "plane_args.h"
#include "region_args.h"
#include "scroll_core.h"
#include "sweep_core.h"

using namespace gg;

namespace {

constexpr int EXPORT_VARIANT_DEFAULT = 0; // gg_export_layers: 0 = k_export_tiled, 1 = k_export_gather; the measured winner
constexpr int IMPORT_VARIANT_DEFAULT = 0; // gg_import_layers: 0 = k_import_tiled, 1 = a batched materialise + k_import_scatter; the measured winner
constexpr int IMAGES_VARIANT_DEFAULT = 0; // gg_export_images: 0 = the tiled kernels of k11_images.hip, 1 = their cell-by-cell forms; the measured winner
constexpr int K_SCORE = GG_NUM_KERNELS; // k_score's entry of the profiler's sums, behind the seven kernels of the path

// one timed kernel of a profiled launch sequence (GG_FLAG_PROFILE).  Consecutive kernels of a sequence SHARE the event between them -- the
// stop of one is the start of the next (owns_start = false): eight events per batch instead of fourteen (the markers cost the 1024-cloud
// step 0.05 ms) -- so a kernel's time includes the few microseconds the stream idles in front of it.
struct EventPair {
    hipEvent_t start, stop;
    int kernel;
    bool owns_start;
};

// A ring of PARAM_RING pinned parameter blocks (each with a device copy): a call takes the next entry, fills it on the host, uploads it and
// records `done` behind the last copy that reads it -- and `done2` on the side stream when the call ran as two halves
// (GG_FLAG_CONCURRENT_HALVES).  acquire() waits on the host for whichever of the two the entry's last user recorded, so a pinned entry is
// rewritten only when the copies that read it have run.
struct ParamRing {
    Event done[PARAM_RING], done2[PARAM_RING];
    bool used[PARAM_RING]{}, used2[PARAM_RING]{};
    int next = 0;
    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < PARAM_RING && e == hipSuccess; ++i) e = done[i].create();
        for (int i = 0; i < PARAM_RING && e == hipSuccess; ++i) e = done2[i].create();
        return e;
    }
    hipError_t acquire(int *g)
    {
        *g = next;
        next = (next + 1) % PARAM_RING;
        hipError_t e = used[*g] ? hipEventSynchronize(done[*g]) : hipSuccess;
        if (e == hipSuccess && used2[*g]) e = hipEventSynchronize(done2[*g]);
        if (e == hipSuccess) used[*g] = used2[*g] = false;
        return e;
    }
    hipError_t recorded(int g, hipStream_t st)
    {
        const hipError_t e = hipEventRecord(done[g], st);
        if (e == hipSuccess) used[g] = true;
        return e;
    }
    hipError_t recorded2(int g, hipStream_t half_stream)
    {
        const hipError_t e = hipEventRecord(done2[g], half_stream);
        if (e == hipSuccess) used2[g] = true;
        return e;
    }
};

// what a many-map call allocates at its first use (alloc_call_scratch): one device block and one pinned host block
struct CallScratch {
    DeviceBlock<char> dev;
    PinnedBlock<char> pinned;
};

// One kind of table that a many-map call sends along in its ring entry: `per_entry` elements for each of the PARAM_RING entries, in the
// call scratch's pinned block and in its device block (RingPart: where, in bytes).  ring_entry() and ring_upload() below use it.
struct RingPart {
    size_t dev, pinned, per_entry;
};
template <typename T>
struct RingTable {
    T *host = nullptr, *dev = nullptr;
    size_t per_entry = 0;
    void bind(const CallScratch &m, const RingPart &p)
    {
        host = (T *)(m.pinned + p.pinned);
        dev = (T *)(m.dev + p.dev);
        per_entry = p.per_entry;
    }
};

} // namespace

struct gg_context : ContextBuffers {
    int device = 0;
    HostHelper helper;
    // the streams come first: members die in reverse order, so a stream outlives every event recorded on it and every block it worked on.
    // h2d / d2h: a copy stream each way for the pipelined host entry point.  half_stream: GG_FLAG_CONCURRENT_HALVES, below
    Stream stream, h2d_stream, d2h_stream, half_stream;
    DeviceBlock<> d_arena; // the one block arena_layout.h lays out: Arena's and ContextBuffers' pointers point into it
    Arena arena{};
    gg_config cfg{};
    gg_geometry geom{};
    int n_slots = 0;
    size_t max_points = 0;
    unsigned flags = 0;
    std::string last_error;

    size_t arena_bytes = 0;
    std::vector<float> h_expected;
    std::vector<double> pos_x, pos_y; // per slot map position
    std::vector<char> slot_seen;      // scratch of check_slot_list
    std::vector<char> no_confidence;  // per slot: groundpatch <= 0.01 everywhere for sure (set by gg_reset_map, cleared by any writer)
    // per slot: the map is FRESH -- gg_reset_maps left the interior of its (ground, confidence) layer unwritten (gg_internal.h Arena::gp_fresh_cell);
    // a batch of at least FRESH_MIN_CLOUDS fresh maps sweeps them as they are, anything else that touches the layer fills it first (make_real)
    std::vector<char> fresh;
    // per slot: the layer's memory may hold a confidence with bit 31 set that is NOT a fresh launch's tag of its own call -- a caller's plane
    // (gg_set_layer, gg_import_layers of groundpatch: negatives, NaN), a stage run on such a layer, a batch that a device-side error cut short.
    // A fresh launch would take such a cell for one k_patch wrote: the slot's next gg_reset_maps fills every cell once and clears the flag.
    // Also set by a batch on a slot whose configuration does not keep k_patch's confidences positive (confidences_stay_positive): such a
    // slot is never swept fresh.  After a device-side error the flags are set when the error is READ (device_error, behind a synchronisation):
    // a reset and batch pipelined behind the voided batch before that belong to the batches the report voids (every batch since the last one).
    std::vector<char> gp_tainted;
    std::vector<float> fresh_z;       // ... and the ground height its cells hold by definition
    bool fresh_enabled = true;        // env GG_FRESH_MAPS=0 / tuning "fresh_maps": gg_reset_maps writes every cell, as before
    // GG_FLAG_MINIMAL_LAYERS: the slot's last cloud left maxGroundHeight / groundCandidates / planeDist unwritten; a reader of one of
    // them has them computed first, from what that call left in the slot's buffers and with its parameters (ensure_lazy_layers)
    bool probe_unordered_streams = false; // measurement only: batches and resets on different caller streams are NOT ordered by the library
    std::vector<char> lazy_pending;
    std::vector<gg::CloudParams> lazy_params;
    // gg_set_slot_configs: per slot, does it have a configuration of its own (else it follows `cfg`), which, and its DevConfig; the device
    // copy (Arena::slot_cfg, entry s = slot s) is allocated at the first call and uploaded whenever the slot configurations change
    std::vector<char> slot_own;
    std::vector<gg_config> slot_cfg;
    std::vector<DevConfig> slot_dev;
    DeviceBlock<DevConfig> d_slot_cfg;
    // the evaluator counters (gg_set_score_labels / gg_set_slot_scoring): one device block, allocated by the first label list -- the ring ->
    // bin table, the slots' on / off bytes, the counters and the 2-bit label masks k_label leaves for k_score when the caller passed none
    // (row = position in the batch, like gg_batch.d_label_masks)
    DeviceBlock<uint8_t> d_score_block;
    gg::ScoreArgs score{};
    uint8_t *d_score_masks = nullptr;
    size_t score_masks_bytes = 0;
    int score_n_ids = 0; // 0: no label list yet
    std::vector<char> score_on;

    gg_conventions conv{};
    gg::sweep::Params sweep_params{};

    // cross-stream ordering (include/groundgrid_hip.h, gg_filter_batch): `map_event` is recorded on ctx->stream after every
    // map mutation enqueued there, `batch_event` on the launch stream after every batch
    Event map_event, batch_event;
    Event gather_event;                      // recorded behind the last gg_allgather_label_masks
    hipStream_t gather_stream = nullptr;
    const uint8_t *gather_lo = nullptr, *gather_hi = nullptr; // ... and the send buffer it reads (null: none pending)
    bool map_event_pending = false;          // a mutation was enqueued on ctx->stream since the last batch waited for it
    hipStream_t last_batch_stream = nullptr; // stream batch_event was last recorded on
    bool have_batch_event = false;
    // GG_FLAG_CONCURRENT_HALVES: the clouds (and map re-initialisations) of the upper half of the slots run on half_stream; half_done is
    // recorded there behind each of them, half_fork on the caller's stream in front (the side stream sees what the caller enqueued before)
    bool layer_copy_failed = false; // a download of the fused filter + layers call could not be enqueued (reported by the call)
    Event half_fork, half_done;
    bool have_half_event = false;
    // Output rows are indexed by a cloud's position in the batch, its half by its slot: two divided batches that are not joined (same caller
    // stream) may write the same row of the same buffer from different streams.  The last few divided batches' output ranges and
    // row-to-half maps are remembered; a batch that shares a range with one of them under another map joins first (enqueue_batch).
    struct HalvesRecord {
        const uint8_t *lo[7] = {}, *hi[7] = {}; // (the seventh: the context's own label masks, when k_score reads them)
        uint64_t map_hash = 0;
    };
    HalvesRecord halves_hist[4];
    int halves_hist_n = 0;
    int halves_min_clouds = 256;
    // gg_filter_cloud / _async / _layers: k_label writes counts, index and labels straight into the pinned host block (posted writes over
    // the link while the kernel runs) instead of into HBM with a copy behind the kernel: one transfer and one stream hop less per call
    int results_direct = 1;
    int upload_pieces = 1; // the input cloud is packed and uploaded in this many pieces (the copy of one travels while the next is packed:
                           // measured 1 / 2 / 3 / 4 pieces: 0.472 / 0.478 / 0.488 / 0.494 ms per synchronous call -- a piece's split and copy
                           // call cost more than its overlap gives)
    bool probe_no_fork = false;

    // pipelined host entry point (gg_filter_cloud_async / _wait): GG_ASYNC_DEPTH staging sets; the device side of set k is async_set[k]
    struct __attribute__((visibility("hidden"))) AsyncSlot {
        PinnedBlock<gg_point16> h_pts;
        PinnedBlock<int32_t> h_counts; // counts, index and labels in one block, like the device's (ContextBuffers::AsyncSet)
        uint8_t *h_labels = nullptr;   // (placed per ticket: behind the n index entries)
        int32_t *h_index = nullptr;
        int32_t *hd_counts = nullptr; // h_counts as the device addresses it (results_direct)
        Event uploaded, computed, downloaded;
        const gg_point32 *cloud = nullptr;
        size_t n = 0;
        bool has_tf = false;
        double tf[12]{};
        int ticket = -1;
    } async_slot[GG_ASYNC_DEPTH];
    int next_ticket = 0, oldest_ticket = 0;
    int slot_of_ticket[GG_ASYNC_DEPTH] = {}; // staging set of an outstanding ticket (a synchronous call always takes set 0)
    int next_label_shift = 0;                // enqueue_ticket -> enqueue_batch: CloudParams::label_shift of the one cloud
    double host_t[4] = {0, 0, 0, 0}; // GG_HOST_TIMING: pack+upload, enqueue, wait, copy-out
    long host_calls = 0;

    // per-call parameter ring (pinned host + device)
    PinnedBlock<CloudParams> h_params; // [PARAM_RING][n_slots], the host side of d_params
    ParamRing ring;

    // staging for the host-buffer entry point, the host side of d_stage_*
    PinnedBlock<gg_point16> h_stage_pts; // [max_points]
    PinnedBlock<uint8_t> h_stage_labels;
    PinnedBlock<int32_t> h_stage_index;
    PinnedBlock<int32_t> h_stage_counts; // [4]
    // gg_move_maps (allocated at its first call; contexts that never call it do not pay): one device block holding the cell table (element,
    // row | col << 16 of every cell in element order), the parameter ring [PARAM_RING][n_slots] and move_cap scratch rows of C cells
    CallScratch move_mem;
    const int2 *d_move_cells = nullptr;
    MoveParams *d_move_params = nullptr, *h_move_params = nullptr; // (h_: pinned, the whole of move_mem.pinned)
    float2 *d_move_scratch = nullptr;
    int move_cap = 0;        // scratch rows: maps per chunk (half of them per stream when the call runs as two halves)
    int move_chunk_tune = 0; // tuning "move_chunk": at most this many maps per chunk (tests: several chunks in a small call)
    ParamRing move_ring;
    // gg_export_layers (allocated at its first call): one device block holding the export table (gg_internal.h PlaneArgs), a ring of map
    // tables [PARAM_RING][n_slots] and a ring of parameter records for the batched launch of the lazily kept layers; their pinned host copies
    // (gg_import_layers runs on the same table, rings and events)
    CallScratch export_mem;
    const uint32_t *d_export_off = nullptr, *d_export_elem = nullptr;
    const uint16_t *d_export_cell = nullptr;
    ExportMap *d_export_maps = nullptr, *h_export_maps = nullptr;
    CloudParams *d_export_lazy = nullptr, *h_export_lazy = nullptr;
    // the tables a plane call sends along in its ring entry (RingTable; laid out by ensure_export_scratch)
    RingTable<int2> ring_shifts;       // gg_fuse_states, gg_track_clusters, gg_match_planes: the per-map index shifts, [n_slots]
    RingTable<int32_t> ring_starts;    // gg_route_planes: the per-map start cells, [n_slots]
    RingTable<int2> ring_pivots;       // gg_match_planes: the per-map pivots, [n_slots]
    RingTable<int2> ring_rotations;    // ... its rotation table, [MATCH_MAX_ROTATIONS]
    MatchPartial *d_match_partials = nullptr; // ... what its two launches hand over, [PARAM_RING][n_slots][MATCH_MAX_ROTATIONS], device only
    RingTable<uint32_t> ring_footprint; // gg_footprint_planes: the packed span table, [FOOTPRINT_TABLE]
    RingTable<uint32_t> ring_moves;    // gg_route_headings: the packed move table, [HEADINGS_TABLE]
    RingTable<int2> ring_poses;        // ... the per-map start (cell, heading), [n_slots]
    RingTable<int32_t> ring_rollout_starts; // gg_score_rollouts: the per-map start (r16, c16, k0), [n_slots][3]
    ParamRing export_ring;
    int slopes_variant = 0; // tuning "slopes_variant": 0 = k_slopes_tiled, 1 = k_slopes_gather (the A/B of tools/bench_slopes.py)
    int export_variant = EXPORT_VARIANT_DEFAULT; // tuning "export_variant": 0 = k_export_tiled, 1 = k_export_gather (the A/B of tools/bench_export.py)
    int import_variant = IMPORT_VARIANT_DEFAULT; // tuning "import_variant": 0 = k_import_tiled, 1 = k_import_scatter (the A/B of tools/bench_import.py)
    // gg_export_images runs on the same table, rings and events; its bounds launch leaves the partial (min, max) pairs of a call in the ring
    // entry's part of d_image_partials: [PARAM_RING][n_slots][GG_NUM_LAYERS][image_parts_cap][2] floats
    float *d_image_partials = nullptr;
    int image_parts_cap = 0;
    int images_variant = IMAGES_VARIANT_DEFAULT; // tuning "images_variant": 0 = the tiled kernels, 1 = cell by cell (the A/B of tools/bench_images.py)
    // gg_split_clouds and gg_rasterize_clouds (allocated at the first call of either): the per-cloud records [PARAM_RING][n_slots] (device
    // and pinned) and the chunk counters of the split's two launches, [PARAM_RING][n_slots][NCH] pairs.  The calls run in the export's frame:
    // an entry of export_ring is an entry here, so they have no ring of their own
    CallScratch split_mem;
    SplitCloud *d_split_clouds = nullptr, *h_split_clouds = nullptr;
    uint2 *d_split_counts = nullptr;
    // gg_cluster_clouds (allocated at its first call): the root counters of its cell launches, [PARAM_RING][n_slots][cluster_cell_chunks]
    // words, in the same frame: an entry of export_ring is an entry here
    CallScratch cluster_mem;
    uint32_t *d_cluster_counts = nullptr;
    int cluster_cell_chunks = 0;
    DeviceBlock<float> d_planes;       // GG_NUM_LAYERS * Cpad floats: dense planes of gg_get_layers (ensure_plane_staging, at first use)
    PinnedBlock<float> h_planes;       // ... and their pinned landing zone on the host (one download for all requested layers)
    DeviceBlock<uint8_t> d_pc2;        // gg_filter_cloud_pc2_out: [64 B counts][max_points * 18 B records], device and pinned host (allocated on first use)
    PinnedBlock<uint8_t> h_pc2;
    PinnedBlock<volatile uint32_t> h_dev_error; // host view of Arena::dev_error (mapped pinned memory)

    // One cloud per call -- the reference's own call shape (src/GroundGridNodelet.cpp:196) -- replays a captured HIP graph: the seven
    // launches (and, for the fused filter + layers call, the layer extraction and downloads on a side branch) are handed to the device
    // as ONE submission.  A captured sequence bakes in everything but the cloud's parameter record, which every replay reads from the
    // same device address (d_gparams, refreshed by a copy in front of the graph): key = what else the launchers were given.
    struct GraphKey {
        BatchIO io;
        int max_n, slot;
        unsigned flags;
        int eigen;
        unsigned long long generation; // bumped by whatever changes the kernels' by-value arguments (configuration, tuning, conventions)
        unsigned layer_mask;           // fused call: layers extracted and downloaded inside the graph ...
        void *layer_dst[GG_NUM_LAYERS]; // ... and where to (pinned staging or the caller's registered planes)
        hipStream_t stream;
    };
    struct GraphEntry {
        GraphKey key;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        int uses = 0;
        unsigned long long last_use = 0;
    };
    std::vector<GraphEntry> graphs;
    unsigned long long graph_generation = 1, graph_clock = 0;
    bool graphs_enabled = false; // opt-in (GG_GRAPH=1, gg_debug_set_tuning("graphs", 1)): measured on MI355X / ROCm 7.0.2 a replay is no faster than the
                                 // seven eager launches -- one cloud, device-resident input: 0.420 against 0.416 ms, the synchronous host call 0.589
                                 // against 0.571 (profiles/r05a/host_call_probe*.json): the launches of a call already queue up behind the first
                                 // kernel, there are no gaps left for a graph to close
    long graph_replays = 0, graph_captures = 0;
    Event fork_event, join_event; // the side branch of the fused filter + layers call
    Event layers_event;           // ... and its late layers (behind the results on the context's stream)
    std::vector<std::pair<char *, size_t>> registered;     // gg_host_register: host ranges downloads may land in directly

    // profiling
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> free_single_events;
    double k_ms[GG_NUM_KERNELS + 1]{}; // (+ k_score, which gg_get_kernel_times' arrays have no room for: gg_get_score_kernel_time)
    int64_t k_launches[GG_NUM_KERNELS + 1]{};

    // gg_cluster_planes (behind everything else: no other member moved for it)
    int32_t *d_region_counts = nullptr;      // [ring entry][map] K, in cluster_mem behind the root counters
    int regions_tile = REGIONS_TILE_DEFAULT; // 1 = the tile-local stage in front of the flatten (gg_debug_regions_tile)
};

namespace {

int fail(gg_context *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess)
            snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else
            snprintf(buf, sizeof buf, "%s", what);
        ctx->last_error = buf;
    }
    return code;
}

int fail(gg_context *ctx, int code, const char *who, const char *what) { return fail(ctx, code, (std::string(who) + ": " + what).c_str()); }

#define HIPCHK(ctx, call)                                                      \
    do {                                                                       \
        hipError_t e__ = (call);                                               \
        if (e__ != hipSuccess) return fail((ctx), GG_ERR_HIP, #call, e__);     \
    } while (0)

// The sign tag of fresh maps (gg_internal.h Arena::gp_fresh_cell) needs every confidence the path writes to be positive.  The sweep's is
// (max(w - w / f, 0.001), unless f is NaN), k_patch's min(old + 0.1, 0.5) is, and its :387 min((sum / (2 * factor) + old) / 2, 1) is for a
// positive, finite occupied_cells_point_count_factor -- nothing else in gg_config enters a confidence.
static bool confidences_stay_positive(const gg_config &c)
{
    return c.occupied_cells_point_count_factor > 0 && std::isfinite((double)c.occupied_cells_point_count_factor) &&
           c.occupied_cells_decrease_factor == c.occupied_cells_decrease_factor;
}

// After a synchronisation: did a kernel give up a bounded wait (Arena::dev_error)?  The reference has no error path at all
// (SURVEY 5); a library that spins inside kernels must at least say so instead of hanging or returning garbage silently.
// The word is read AND cleared here: the report is about the batches enqueued since the last report -- their outputs are void, the
// map states they touched should be re-initialised (gg_reset_map) -- and the context goes on working (a sticky word turned one
// spurious timeout into GG_ERR_HIP from every later call, gg_reset_map + gg_synchronize included).
int device_error(gg_context *ctx)
{
    const uint32_t code = ctx->h_dev_error ? *ctx->h_dev_error : 0u;
    if (code == GG_DEVERR_NONE) return GG_OK;
    *ctx->h_dev_error = GG_DEVERR_NONE;
    std::fill(ctx->gp_tainted.begin(), ctx->gp_tainted.end(), (char)1); // (a fresh launch cut short may have left tagged confidences behind)
    return fail(ctx, GG_ERR_HIP, code == GG_DEVERR_FRONT_WAIT ? "k_classify: a cloud's tile scan never completed (bounded wait ran out); the outputs of that batch are void"
                                 : code == GG_DEVERR_SCAN_WAIT ? "k_scan: the sums of an earlier part of a cloud never arrived (bounded wait ran out); the outputs of that batch are void"
                                 : code == GG_DEVERR_SWEEP_WAIT ? "k_sweep: a hand-over between work-groups never arrived (bounded wait ran out); the outputs of that batch are void"
                                                                : "a kernel reported an unknown device-side error");
}
#define SYNCCHK(ctx, call)                                   \
    do {                                                     \
        HIPCHK(ctx, call);                                   \
        const int rc__ = device_error(ctx);                  \
        if (rc__ != GG_OK) return rc__;                      \
    } while (0)

// an integer knob of the environment (atoi: text that is no number reads as 0); `fallback` when the variable is not set
int env_int(const char *name, int fallback)
{
    const char *v = getenv(name);
    return v ? atoi(v) : fallback;
}

uint32_t morton2(uint32_t x, uint32_t y)
{
    auto spread = [](uint32_t v) {
        v &= 0xFFFFu;
        v = (v | (v << 8)) & 0x00FF00FFu;
        v = (v | (v << 4)) & 0x0F0F0F0Fu;
        v = (v | (v << 2)) & 0x33333333u;
        v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    return spread(x) | (spread(y) << 1);
}

void make_dev_config(const gg_config &c, DevConfig &d)
{
    d.point_count_cell_variance_threshold = c.point_count_cell_variance_threshold;
    d.max_ring = c.max_ring;
    d.outlier_tolerance = c.outlier_tolerance;
    d.gpd_min_point_count_threshold = c.ground_patch_detection_minimum_point_count_threshold;
    d.patch_size_change_distance_sq = c.patch_size_change_distance * c.patch_size_change_distance; // pow(x, 2.0)
    d.occupied_cells_decrease_factor = c.occupied_cells_decrease_factor;
    d.occupied_cells_point_count_factor = c.occupied_cells_point_count_factor;
    d.occupied_cells_point_count_factor_x2 = c.occupied_cells_point_count_factor * (double)2.0f; // :387
    d.min_outlier_detection_ground_confidence = c.min_outlier_detection_ground_confidence;
    d.distance_factor_sq = c.distance_factor * c.distance_factor;                                 // :369
    d.minimum_distance_factor_sq = c.minimum_distance_factor * c.minimum_distance_factor;
    const double m10 = c.minimum_distance_factor * 10;
    d.minimum_distance_factor_x10_sq = m10 * m10;
    d.min_dist_fac = c.minimum_distance_factor * 5; // :154
    d.min_point_height_thres = c.miminum_point_height_threshold;
    d.min_point_height_obs_thres = c.minimum_point_height_obstacle_threshold;
    d.inv_decrease = 1.0 / c.occupied_cells_decrease_factor;                                        // (launch_sequence's sweep::Params)
    d.decay_fast = c.occupied_cells_decrease_factor >= 1.25 && c.occupied_cells_decrease_factor < 1e300 ? 1 : 0;
}

hipStream_t pick_stream(gg_context *ctx, void *stream)
{
    if (stream == GG_STREAM_DEFAULT) return (hipStream_t) nullptr; // the legacy default stream
    return stream ? (hipStream_t)stream : ctx->stream;
}

// `st` follows the half of every earlier batch that ran on the library's side stream (GG_FLAG_CONCURRENT_HALVES)
int stream_waits_for_second_half(gg_context *ctx, hipStream_t st)
{
    if (ctx->have_half_event && st != ctx->half_stream) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->half_done, 0));
    return GG_OK;
}
// Entry points that read or write map state on ctx->stream call this first: the context's stream waits for the last batch
// that ran on another stream (gg_get_layer after a batch on a caller stream read stale layers).
// FRESH maps (gg_context::fresh) among the slots [first, first + n) become real on stream `st`: the fill gg_reset_maps left out (:71-75).
// The caller has ordered `st` behind the reset.
int make_real(gg_context *ctx, int first, int n, hipStream_t st)
{
    const Arena &a = ctx->arena;
    for (int s = first; s < first + n;) {
        if (!ctx->fresh[s]) {
            ++s;
            continue;
        }
        int e = s + 1;
        while (e < first + n && ctx->fresh[e] && ctx->fresh_z[e] == ctx->fresh_z[s]) ++e; // one strided fill per run of equal heights
        launch_fill2_strided(gp2_ptr(a, s), (size_t)a.gpl.elems, a.gp2_stride, e - s, ctx->fresh_z[s], (float)0.0000001, a.gp_valid, st);
        for (int k = s; k < e; ++k) ctx->fresh[k] = 0;
        s = e;
    }
    HIPCHK(ctx, hipGetLastError());
    return GG_OK;
}

// (maps_real = false: the caller touches no layer -- a re-initialisation leaves the other maps as they are)
int own_stream_waits_for_batches(gg_context *ctx, bool maps_real = true)
{
    if (ctx->have_batch_event && ctx->last_batch_stream != ctx->stream)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->batch_event, 0));
    if (const int rc = stream_waits_for_second_half(ctx, ctx->stream)) return rc;
    if (!maps_real) return GG_OK;
    // whatever the context's own stream does next with map state (getters, setters, scrolls, stages, single clouds) finds real layers
    bool any = false;
    for (int s = 0; s < ctx->n_slots && !any; ++s) any = ctx->fresh[s] != 0;
    if (!any) return GG_OK;
    if (const int rc = make_real(ctx, 0, ctx->n_slots, ctx->stream)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->map_event, ctx->stream)); // (own_stream_mutated_map: a batch on another stream waits for the fill)
    ctx->map_event_pending = true;
    return GG_OK;
}
// ... and this after enqueueing a mutation of map state on ctx->stream (reset, move, set_layer): the next batch on any
// other stream waits for it.
int own_stream_mutated_map(gg_context *ctx)
{
    HIPCHK(ctx, hipEventRecord(ctx->map_event, ctx->stream));
    ctx->map_event_pending = true;
    return GG_OK;
}

// The ordering pair of the many-map calls (gg_reset_maps, gg_move_maps, gg_export_layers, gg_import_layers) on stream `st`.
// call_follows_context, in front of what the call enqueues: `st` follows every earlier map mutation, batch and second half of the context.
// call_recorded, behind it: whatever touches these maps next on another stream waits for the call.
//                      skip_half_join                                        clears_map_pending
//   gg_reset_maps      the call is itself divided into the two halves        false
//   gg_move_maps       the call is itself divided into the two halves        false
//   gg_export_layers   false (it reads maps of either half)                  true
//   gg_import_layers   false (it writes maps of either half)                 true
// skip_half_join: a divided call right behind a batch (or divided call) on the same caller stream does not wait for the side stream -- a slot
// is only ever touched from its half's stream, so the halves of consecutive calls need not meet (as in enqueue_batch).
// clears_map_pending: on a caller stream, `st` has waited for map_event and later batches anywhere follow batch_event, so the pending mark
// is dropped (as enqueue_batch does).  Reset and move leave it set, which costs the next batch on another stream one wait for an event that
// batch_event already implies.
// (enqueue_batch keeps its own prologue and epilogue: it joins the halves by its output-row history, applies probe_unordered_streams on the
// context's stream too and records batch_event there as well)
int call_follows_context(gg_context *ctx, hipStream_t st, bool skip_half_join)
{
    if (st == ctx->stream) return own_stream_waits_for_batches(ctx, false);
    if (ctx->map_event_pending) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->map_event, 0));
    if (ctx->have_batch_event && ctx->last_batch_stream != st && !ctx->probe_unordered_streams) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->batch_event, 0));
    if (skip_half_join && ctx->last_batch_stream == st) return GG_OK;
    return stream_waits_for_second_half(ctx, st);
}
int call_recorded(gg_context *ctx, hipStream_t st, bool clears_map_pending)
{
    if (st == ctx->stream) return own_stream_mutated_map(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->batch_event, st));
    ctx->have_batch_event = true;
    ctx->last_batch_stream = st;
    if (clears_map_pending) ctx->map_event_pending = false;
    return GG_OK;
}

// rocTX ranges named after the reference's four stage timers (src/GroundSegmentation.cpp:124 "rasterization", :138 "patch
// detection", :144 "interpolation", :194 "segmentation") around the launch groups of a batch, so that a rocprofv3
// --marker-trace reads in the reference's terms.  The library is looked up at run time (no link-time dependency, nothing happens
// when no profiler is attached); GG_ROCTX=0 turns it off.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        if (env_int("GG_ROCTX", 1) == 0) return;
        for (const char *name : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "libroctx64.so"}) {
            void *h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (!h) continue;
            push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr;
            pop = nullptr;
        }
    }
};
struct StageRange {
    static Roctx &lib()
    {
        static Roctx r;
        return r;
    }
    bool on;
    explicit StageRange(const char *stage) : on(lib().push != nullptr)
    {
        if (on) lib().push(stage);
    }
    ~StageRange()
    {
        if (on) lib().pop();
    }
    StageRange(const StageRange &) = delete;
};

struct Profiler {
    gg_context *ctx;
    hipStream_t s;
    bool on;
    EventPair cur{};
    hipEvent_t prev = nullptr; // the stop event of the kernel before, recorded on `s` by this sequence
    hipEvent_t take()
    {
        hipEvent_t e = nullptr;
        if (!ctx->free_single_events.empty()) {
            e = ctx->free_single_events.back();
            ctx->free_single_events.pop_back();
        } else
            hipEventCreate(&e);
        return e;
    }
    void begin(int k)
    {
        if (!on) return;
        cur.kernel = k;
        cur.owns_start = prev == nullptr;
        if (prev)
            cur.start = prev;
        else {
            cur.start = take();
            hipEventRecord(cur.start, s);
        }
    }
    void end()
    {
        if (!on) return;
        cur.stop = take();
        hipEventRecord(cur.stop, s);
        ctx->pending.push_back(cur);
        prev = cur.stop;
    }
};

int drain_profile(gg_context *ctx)
{
    for (auto &p : ctx->pending) {
        HIPCHK(ctx, hipEventSynchronize(p.stop));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, p.start, p.stop));
        ctx->k_ms[p.kernel] += ms;
        ctx->k_launches[p.kernel] += 1;
    }
    for (auto &p : ctx->pending) { // (a shared event is the stop of exactly one entry)
        if (p.owns_start) ctx->free_single_events.push_back(p.start);
        ctx->free_single_events.push_back(p.stop);
    }
    ctx->pending.clear();
    return GG_OK;
}

// the profiler's events are shared between neighbouring pairs (owns_start) and pooled, so they stay raw handles: gg_destroy releases them here
void release_profile_events(gg_context *ctx)
{
    for (auto &p : ctx->pending) {
        if (p.owns_start) hipEventDestroy(p.start);
        hipEventDestroy(p.stop);
    }
    for (hipEvent_t e : ctx->free_single_events) hipEventDestroy(e);
    ctx->pending.clear();
    ctx->free_single_events.clear();
}

// the record of one plane call (gg_internal.h); the table is null until gg_export_layers / gg_import_layers built it -- only their tiled kernels read it
PlaneArgs fill_plane_args(const gg_context *ctx, const ExportMap *dm, unsigned layer_mask, int order, float *d_planes, size_t plane_stride)
{
    PlaneArgs x;
    x.maps = dm;
    x.block_off = ctx->d_export_off;
    x.elem = ctx->d_export_elem;
    x.cell = ctx->d_export_cell;
    x.blocks_r = (ctx->arena.g.rows + EXPORT_TILE - 1) / EXPORT_TILE;
    x.blocks_c = (ctx->arena.g.cols + EXPORT_TILE - 1) / EXPORT_TILE;
    x.mask = layer_mask;
    x.n_planes = __builtin_popcount(layer_mask);
    x.order = order;
    x.planes = d_planes;
    x.plane_stride = plane_stride;
    return x;
}

// Before anything reads (or densifies) one of the three layers GG_FLAG_MINIMAL_LAYERS leaves out: compute them for this slot, once,
// on the context's stream (the callers have ordered it behind the batches).  SURVEY Appendix E: the published-only layers are
// materialised when somebody asks, from the retained tile-sorted records; gg_get_layer returns at all times what the reference holds.
int ensure_lazy_layers(gg_context *ctx, int slot, bool wanted)
{
    if (!wanted || !ctx->lazy_pending[slot]) return GG_OK;
    launch_reduce_lazy(ctx->arena, ctx->lazy_params[slot], ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    ctx->lazy_pending[slot] = 0;
    return GG_OK;
}
constexpr unsigned LAZY_LAYERS = (1u << GG_LAYER_MAXGROUNDHEIGHT) | (1u << GG_LAYER_GROUNDCANDIDATES) | (1u << GG_LAYER_PLANEDIST);

// The single-map getters and setters: the layers of `mask` of one slot as dense column-major planes at d_dst on `st` (plane k = the k-th set
// bit, `plane_stride` floats apart), and the inverse.  A list of one map for the cell-by-cell kernels of the many-map calls (k6_wire.hip).
int extract_planes(gg_context *ctx, int slot, unsigned mask, float *d_dst, size_t plane_stride, hipStream_t st)
{
    if (const int rc = ensure_lazy_layers(ctx, slot, (mask & LAZY_LAYERS) != 0u)) return rc;
    launch_planes_gather(ctx->arena, fill_plane_args(ctx, ctx->d_slot_maps + slot, mask, GG_PLANES_COLMAJOR, d_dst, plane_stride), 1, st);
    return GG_OK;
}
// (a per-call layer named: all nine become dense first -- they share one set of liveness words, gg_internal.h tile_live -- so the three
// GG_FLAG_MINIMAL_LAYERS left out are computed while their cloud's half columns are still known)
int insert_planes(gg_context *ctx, int slot, unsigned mask, const float *d_src, size_t plane_stride, hipStream_t st)
{
    if (const int rc = ensure_lazy_layers(ctx, slot, (mask & ~((1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH))) != 0u)) return rc;
    launch_planes_scatter(ctx->arena, fill_plane_args(ctx, ctx->d_slot_maps + slot, mask, GG_PLANES_COLMAJOR, const_cast<float *>(d_src), plane_stride), 1, st);
    return GG_OK;
}

// layers the fused filter + layers call (gg_filter_cloud_layers) extracts and downloads inside the launch sequence
struct LayerPlan {
    unsigned mask = 0u;                 // bit per gg_layer
    void *dst[GG_NUM_LAYERS] = {};      // where layer l lands: the caller's registered plane, or its plane of the pinned staging block
};
// the eight per-call layers that are final once k_reduce has run (K3 / K4 / K5 only read them; `points` is rewritten by K4 / K5,
// ground / groundpatch by K3 / K4): their extraction and download overlap the terrain sweep on a side branch
constexpr unsigned EARLY_LAYERS = (1u << GG_LAYER_MINGROUNDHEIGHT) | (1u << GG_LAYER_MAXGROUNDHEIGHT) | (1u << GG_LAYER_GROUNDCANDIDATES) | (1u << GG_LAYER_PLANEDIST) |
                                  (1u << GG_LAYER_M2) | (1u << GG_LAYER_MEANVARIANCE) | (1u << GG_LAYER_POINTSRAW) | (1u << GG_LAYER_VARIANCE);

// extraction kernel + one download per layer of `mask` on stream `st`.  The early group owns planes 0..7 of d_planes, the late group
// (ground, groundpatch, points) planes 8..10: the two never share one.
void enqueue_layer_downloads(gg_context *ctx, const Arena &a, int slot, unsigned mask, const LayerPlan &plan, hipStream_t st)
{
    if (!mask) return;
    const size_t plane = align_up((size_t)a.g.C * 4, 256) / 4;
    float *base = ctx->d_planes + (size_t)((mask & EARLY_LAYERS) ? 0 : 8) * plane;
    (void)extract_planes(ctx, slot, mask, base, plane, st); // (no layer is owed here: the batch in front of it computed all nine)
    int k = 0;
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!((mask >> l) & 1u)) continue;
        if (hipMemcpyAsync(plan.dst[l], base + (size_t)k * plane, (size_t)a.g.C * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) ctx->layer_copy_failed = true;
        ++k;
    }
}

// the kernels of one batched filter_cloud call (and the layer branch of the fused call), on stream s
// score: some cloud's slot keeps evaluator counters (io.d_label_masks is set then): k_score follows the label loop
void launch_sequence(gg_context *ctx, const Arena &a, const CloudParams *dp, const BatchIO &io, int nb, int max_n, hipStream_t s, const LayerPlan *plan, int slot0,
                     bool profile, bool score)
{
    Profiler prof{ctx, s, profile};
    {
        StageRange stage("rasterization"); // insert_cloud, :98-124
        // the front end in one, two or three launches (k1_classify.hip): what launch_classify did not do itself follows here
        prof.begin(GG_K_CLASSIFY);
        const int front = launch_classify(a, dp, io, nb, max_n, s);
        prof.end();
        if (front == FRONT_THREE_LAUNCHES) {
            prof.begin(GG_K_SCAN);
            launch_scan(a, dp, nb, s);
            prof.end();
        }
        if (front != FRONT_ONE_LAUNCH) {
            prof.begin(GG_K_SCATTER);
            launch_scatter(a, dp, nb, max_n, s);
            prof.end();
        }
        prof.begin(GG_K_REDUCE);
        launch_reduce(a, dp, nb, s);
        prof.end();
    }
    const bool side = plan && (plan->mask & EARLY_LAYERS);
    if (side) { // fork: the layers k_reduce has just finished travel while the stencil and the sweep run
        hipEventRecord(ctx->fork_event, s);
        hipStreamWaitEvent(ctx->d2h_stream, ctx->fork_event, 0);
        enqueue_layer_downloads(ctx, a, slot0, plan->mask & EARLY_LAYERS, *plan, ctx->d2h_stream);
        hipEventRecord(ctx->join_event, ctx->d2h_stream);
    }
    {
        StageRange stage("patch detection"); // detect_ground_patches, :126-138
        prof.begin(GG_K_PATCH);
        launch_patch(a, dp, nb, s);
        prof.end();
    }
    prof.begin(GG_K_SPIRAL);
    {
        StageRange stage("interpolation"); // spiral_ground_interpolation, :141-144
        sweep::Params sp = ctx->sweep_params;
        sp.decrease = ctx->cfg.occupied_cells_decrease_factor;
        sp.inv_decrease = 1.0 / sp.decrease;
        sp.decay_fast = sp.decrease >= 1.25 && sp.decrease < 1e300;
        launch_sweep(a, sp, dp, nb, s, ctx->d_sweep_dbg);
    }
    prof.end();
    {
        StageRange stage("segmentation"); // the label loop, :146-194
        prof.begin(GG_K_LABEL);
        launch_label(a, dp, io, nb, max_n, s);
        prof.end();
        if (score) { // scripts/eval_groundpoint_classifier.py:95-132
            prof.begin(K_SCORE);
            launch_score(a, dp, io, ctx->score, nb, max_n, s);
            prof.end();
        }
    }
    if (side) hipStreamWaitEvent(s, ctx->join_event, 0); // join (the late layers -- ground, groundpatch, points -- follow the results: enqueue_ticket)
}

void drop_graphs(gg_context *ctx)
{
    for (auto &e : ctx->graphs) {
        if (e.exec) hipGraphExecDestroy(e.exec);
        if (e.graph) hipGraphDestroy(e.graph);
    }
    ctx->graphs.clear();
}

// One cloud per call replays a captured graph (gg_context::GraphKey); everything else, and the first call of a kind, launches eagerly.
int launch_or_replay(gg_context *ctx, const Arena &a, const CloudParams *hp, CloudParams *dp, const BatchIO &io, int nb, int max_n, hipStream_t s, const LayerPlan *plan,
                     bool score)
{
    const bool profile = (ctx->flags & GG_FLAG_PROFILE) != 0;
    // (the fused filter + layers call stays eager: its side branch runs on a second stream beside the sweep, and a captured graph
    // executed the branch's nodes one after the other -- 0.77 against 0.72 ms per call, profiles/r05a)
    const bool eligible = nb == 1 && !plan && ctx->graphs_enabled && !profile && !ctx->d_sweep_dbg && s != nullptr && !a.k2_debug && !a.k3_debug && !a.k5_debug && !a.k2_skip;
    if (!eligible) {
        HIPCHK(ctx, hipMemcpyAsync(dp, hp, sizeof(CloudParams) * nb, hipMemcpyHostToDevice, s));
        launch_sequence(ctx, a, dp, io, nb, max_n, s, plan, hp[0].slot, profile, score);
        return GG_OK;
    }
    gg_context::GraphKey key;
    memset(&key, 0, sizeof key); // (padding included: keys are compared bytewise)
    key.io = io;
    // the grids of a captured sequence cover the largest cloud the buffers can hold: work-groups beyond this cloud's chunks leave at once
    key.max_n = (int)std::min(ctx->max_points, io.cloud_stride);
    key.slot = hp[0].slot;
    key.flags = a.flags;
    key.eigen = a.eigen_reduction;
    key.generation = ctx->graph_generation;
    key.stream = s;
    if (plan) {
        key.layer_mask = plan->mask & EARLY_LAYERS; // (what the captured sequence itself downloads)
        for (int l = 0; l < GG_NUM_LAYERS; ++l) key.layer_dst[l] = ((key.layer_mask >> l) & 1u) ? plan->dst[l] : nullptr;
    }
    gg_context::GraphEntry *entry = nullptr;
    for (auto &e : ctx->graphs)
        if (memcmp(&e.key, &key, sizeof key) == 0) entry = &e;
    if (!entry) {
        if (ctx->graphs.size() >= 8) { // evict the least recently used
            size_t victim = 0;
            for (size_t k = 1; k < ctx->graphs.size(); ++k)
                if (ctx->graphs[k].last_use < ctx->graphs[victim].last_use) victim = k;
            if (ctx->graphs[victim].exec) hipGraphExecDestroy(ctx->graphs[victim].exec);
            if (ctx->graphs[victim].graph) hipGraphDestroy(ctx->graphs[victim].graph);
            ctx->graphs.erase(ctx->graphs.begin() + (long)victim);
        }
        ctx->graphs.emplace_back();
        entry = &ctx->graphs.back();
        entry->key = key;
    }
    entry->last_use = ++ctx->graph_clock;
    // the parameter record of THIS cloud, at the address every capture reads it from (stream order: behind the previous replay)
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_gparams, hp, sizeof(CloudParams), hipMemcpyHostToDevice, s));
    if (entry->exec) {
        HIPCHK(ctx, hipGraphLaunch(entry->exec, s));
        ++ctx->graph_replays;
        return GG_OK;
    }
    if (entry->uses++ == 0) { // first call of a kind: eager (per-device one-time settings of the launchers happen here, outside any capture)
        launch_sequence(ctx, a, ctx->d_gparams, io, 1, key.max_n, s, plan, key.slot, false, score);
        return GG_OK;
    }
    HIPCHK(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    launch_sequence(ctx, a, ctx->d_gparams, io, 1, key.max_n, s, plan, key.slot, false, score);
    hipGraph_t graph = nullptr;
    const hipError_t e_end = hipStreamEndCapture(s, &graph);
    if (e_end != hipSuccess || !graph) {
        (void)hipGetLastError();
        ctx->graphs_enabled = false; // (a runtime that cannot capture this sequence: stay eager)
        launch_sequence(ctx, a, ctx->d_gparams, io, 1, key.max_n, s, plan, key.slot, false, score);
        return GG_OK;
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess || !exec) {
        (void)hipGetLastError();
        hipGraphDestroy(graph);
        ctx->graphs_enabled = false;
        launch_sequence(ctx, a, ctx->d_gparams, io, 1, key.max_n, s, plan, key.slot, false, score);
        return GG_OK;
    }
    entry->graph = graph;
    entry->exec = exec;
    ++ctx->graph_captures;
    HIPCHK(ctx, hipGraphLaunch(exec, s));
    ++ctx->graph_replays;
    return GG_OK;
}

bool slot_ok(const gg_context *ctx, int slot) { return ctx && slot >= 0 && slot < ctx->n_slots; }

// The slots a call names -- slots[0 .. n), or the run first_slot .. first_slot + n - 1 when `slots` is null --: GG_ERR_CAPACITY for one
// outside the context, GG_ERR_INVALID for one named twice, whichever comes first in the list (gg_context::slot_seen is the scratch)
int check_slot_list(gg_context *ctx, const char *who, int n, const int32_t *slots, int first_slot)
{
    if (!slots) // (a run names no slot twice)
        return first_slot < 0 || (long long)first_slot + n > ctx->n_slots ? fail(ctx, GG_ERR_CAPACITY, who, "slot outside the context") : GG_OK;
    ctx->slot_seen.assign((size_t)ctx->n_slots, 0);
    for (int k = 0; k < n; ++k) {
        if (slots[k] < 0 || slots[k] >= ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "slot outside the context");
        if (ctx->slot_seen[(size_t)slots[k]]++) return fail(ctx, GG_ERR_INVALID, who, "a slot is named twice");
    }
    return GG_OK;
}
inline int slot_of(const int32_t *slots, int first_slot, int i) { return slots ? slots[i] : first_slot + i; }

// which half of a context's slots a map belongs to (GG_FLAG_CONCURRENT_HALVES): the upper half runs on the library's side stream
bool second_half_slot(const gg_context *ctx, int slot) { return slot >= (ctx->n_slots + 1) / 2; }
bool halves_enabled(const gg_context *ctx)
{
    return (ctx->flags & GG_FLAG_CONCURRENT_HALVES) && !(ctx->flags & GG_FLAG_PROFILE) && !ctx->d_sweep_dbg && !ctx->arena.k2_debug && ctx->half_stream;
}

// enqueue the seven kernels of one batched filter_cloud call
// batch_entry: the call is gg_filter_batch (device-resident clouds, no layer asked for): the three published-only layers are left to
// their first reader unless GG_FLAG_EAGER_LAYERS says otherwise
int enqueue_batch(gg_context *ctx, const gg_batch *b, hipStream_t s, const LayerPlan *plan = nullptr, bool batch_entry = false)
{
    const bool lazy = (ctx->flags & GG_FLAG_MINIMAL_LAYERS) || (batch_entry && !(ctx->flags & GG_FLAG_EAGER_LAYERS));
    const unsigned eff_flags = lazy ? (ctx->flags | GG_FLAG_MINIMAL_LAYERS) : (ctx->flags & ~(unsigned)GG_FLAG_MINIMAL_LAYERS);
    const int nb = b->n_clouds;
    if (nb == 0) return GG_OK;
    // parameter ring slot
    int g;
    HIPCHK(ctx, ctx->ring.acquire(&g));
    CloudParams *hp = ctx->h_params + (size_t)g * ctx->n_slots;
    CloudParams *dp = ctx->d_params + (size_t)g * ctx->n_slots;
    // Two halves side by side?  The clouds of the lower slots first in the parameter array, then the others: each half is a batch of its own
    int n_first = nb;
    // (not on the legacy default stream: its implicit synchronisation with every other stream makes the two halves slower than one
    // sequence -- 5.75 against 5.29 ms per 1024 clouds, profiles/r05a/halves_probe_default_stream.json)
    const bool split_wanted = halves_enabled(ctx) && !plan && nb >= ctx->halves_min_clouds && s != ctx->half_stream && s != nullptr;
    if (split_wanted) {
        n_first = 0;
        for (int i = 0; i < nb; ++i) n_first += second_half_slot(ctx, slot_of(b->slots, b->first_slot, i)) ? 0 : 1;
    }
    const bool split = split_wanted && n_first > 0 && n_first < nb;
    if (!split) n_first = nb;
    int max_n[2] = {0, 0}, at[2] = {0, n_first};
    for (int i = 0; i < nb; ++i) {
        const int slot = slot_of(b->slots, b->first_slot, i);
        const int half = split && second_half_slot(ctx, slot) ? 1 : 0;
        CloudParams &p = hp[at[half]++];
        p.slot = slot;
        p.n_points = b->n_points[i];
        p.ox = b->origins[i * 3 + 0];
        p.oy = b->origins[i * 3 + 1];
        p.oz = b->origins[i * 3 + 2];
        p.base_z = (float)b->base_z[i];
        p.pos_x = ctx->pos_x[slot];
        p.pos_y = ctx->pos_y[slot];
        p.has_tf = b->transforms ? 1 : 0;
        p.no_confidence = ctx->no_confidence[slot] ? 1 : 0;
        p.fresh = 0;
        ctx->no_confidence[slot] = 0; // the sweep of this call writes confidences
        for (int k = 0; k < 12; ++k) p.tf[k] = b->transforms ? b->transforms[(size_t)i * 12 + k] : 0.0;
        p.label_shift = nb == 1 ? ctx->next_label_shift : 0;
        p.io_index = i;
        p.cfg_index = ctx->slot_own[slot] ? slot : -1;
        if (!confidences_stay_positive(ctx->slot_own[slot] ? ctx->slot_cfg[slot] : ctx->cfg)) ctx->gp_tainted[slot] = 1; // (filled first below, and by its next reset)
        max_n[half] = std::max(max_n[half], p.n_points);
        ctx->lazy_pending[slot] = lazy ? 1 : 0;
        if (lazy) ctx->lazy_params[slot] = p;
    }
    // a (half) launch with a scoring slot is followed by k_score, which reads the labels as the 2-bit masks k_label writes: into the
    // caller's d_label_masks, or into the context's own when there are none; any other launch runs what it always ran
    bool score_half[2] = {false, false};
    if (ctx->score_n_ids)
        for (int i = 0; i < nb; ++i) score_half[i < n_first ? 0 : 1] |= ctx->score_on[hp[i].slot] != 0;
    const bool own_masks = (score_half[0] || score_half[1]) && !b->d_label_masks;
    // FRESH maps (gg_context::fresh): a (half) launch whose maps are all fresh, and large enough for the plain k_sweep, takes them as they
    // are -- k_patch tags what it writes, the sweep takes nothing else of the layer as it is --; in any other launch they are filled first
    bool fresh_half[2] = {false, false};
    for (int h = 0; h < (split ? 2 : 1); ++h) {
        const int lo = h ? n_first : 0, hi = h ? nb : n_first;
        bool all = ctx->fresh_enabled && !plan && !ctx->d_sweep_dbg && sweep_takes_fresh(ctx->arena, ctx->sweep_params, hi - lo);
        for (int i = lo; i < hi && all; ++i) all = ctx->fresh[hp[i].slot] != 0 && !ctx->gp_tainted[hp[i].slot];
        fresh_half[h] = all;
        if (all)
            for (int i = lo; i < hi; ++i) hp[i].fresh = 1, ctx->fresh[hp[i].slot] = 0;
    }
    auto fill_fresh = [&](int lo, int hi, hipStream_t on) -> int { // (the stream is ordered behind the reset by now)
        for (int i = lo; i < hi;) { // one fill per run of consecutive slots (make_real cuts a run where the heights differ)
            int e = i + 1;
            while (e < hi && hp[e].slot == hp[e - 1].slot + 1) ++e;
            if (const int rc = make_real(ctx, hp[i].slot, e - i, on)) return rc;
            i = e;
        }
        return GG_OK;
    };
    // order this batch after everything that touched map state on the context's stream, and after an earlier batch that ran
    // on another stream
    if (s != ctx->stream && ctx->map_event_pending) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->map_event, 0));
    if (ctx->have_batch_event && ctx->last_batch_stream != s && !ctx->probe_unordered_streams) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->batch_event, 0));
    // ... and after the second half of earlier batches -- unless this one is divided the same way: a slot is only ever touched from its
    // half's stream, so the halves of consecutive batches on one caller stream need not meet
    bool joined = false;
    if (!(split && ctx->last_batch_stream == s)) {
        if (const int rc = stream_waits_for_second_half(ctx, s)) return rc;
        joined = true;
    }
    if (split) {
        // ... but the halves of consecutive batches DO meet in the output buffers when a row changes its half (rows follow the batch
        // position, halves the slot): join the two streams once, in both directions, before such a batch
        gg_context::HalvesRecord now;
        const size_t per = b->cloud_stride;
        const uint8_t *p6[7] = {(const uint8_t *)b->d_labels, (const uint8_t *)b->d_out_index, (const uint8_t *)b->d_out_clouds, (const uint8_t *)b->d_out_counts,
                                (const uint8_t *)b->d_label_masks, (const uint8_t *)b->d_out_pc2, own_masks ? ctx->d_score_masks : nullptr};
        const size_t bytes6[7] = {(size_t)nb * per, (size_t)nb * per * 4, (size_t)nb * per * sizeof(gg_point32), (size_t)nb * 64, (size_t)nb * ((per + 3) / 4), (size_t)nb * per * 18,
                                  (size_t)nb * ((per + 3) / 4)};
        for (int k = 0; k < 7; ++k) now.lo[k] = p6[k], now.hi[k] = p6[k] ? p6[k] + bytes6[k] : nullptr;
        uint64_t h = 1469598103934665603ull;
        for (int i = 0; i < nb; ++i) h = (h ^ (uint64_t)(second_half_slot(ctx, slot_of(b->slots, b->first_slot, i)) ? 2 * i + 1 : 2 * i)) * 1099511628211ull;
        now.map_hash = h ^ (uint64_t)nb;
        bool clash = false;
        for (int r = 0; r < ctx->halves_hist_n && !joined && !clash; ++r) {
            const gg_context::HalvesRecord &o = ctx->halves_hist[r];
            if (o.map_hash == now.map_hash) continue; // every row on the stream it was on: ordered by the streams themselves
            for (int x = 0; x < 7 && !clash; ++x)
                for (int y = 0; y < 7 && !clash; ++y) clash = now.lo[x] && o.lo[y] && now.lo[x] < o.hi[y] && o.lo[y] < now.hi[x];
        }
        if (clash) {
            if (const int rc = stream_waits_for_second_half(ctx, s)) return rc;
            if (ctx->have_batch_event) HIPCHK(ctx, hipStreamWaitEvent(ctx->half_stream, ctx->batch_event, 0));
            joined = true;
        }
        if (joined) ctx->halves_hist_n = 0; // (everything before is ordered on both streams now)
        if (ctx->halves_hist_n == 4) {
            for (int r = 1; r < 4; ++r) ctx->halves_hist[r - 1] = ctx->halves_hist[r];
            ctx->halves_hist_n = 3;
        }
        ctx->halves_hist[ctx->halves_hist_n++] = now;
    } else if (joined)
        ctx->halves_hist_n = 0;
    if (ctx->gather_lo) { // an all-gather still reads label masks: a batch on another stream that rewrites them waits for it
        auto overlaps = [&](const uint8_t *p, size_t bytes) { return p && p < ctx->gather_hi && p + bytes > ctx->gather_lo; };
        const size_t per_cloud = b->cloud_stride;
        const bool hit = overlaps(b->d_label_masks, (size_t)nb * ((per_cloud + 3) / 4)) || overlaps(b->d_labels, (size_t)nb * per_cloud);
        if (ctx->gather_stream != s && hit) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->gather_event, 0));
        if (split && hit) HIPCHK(ctx, hipStreamWaitEvent(ctx->half_stream, ctx->gather_event, 0));
        if (ctx->gather_stream == s || hit) ctx->gather_lo = ctx->gather_hi = nullptr; // (ordered now, by the stream or by the event)
    }

    BatchIO io;
    io.d_points = b->d_points;
    io.cloud_stride = b->cloud_stride;
    io.point_format = b->point_format;
    io.d_labels = b->d_labels;
    io.d_out_index = b->d_out_index;
    io.d_out_clouds = b->d_out_clouds;
    io.d_out_counts = b->d_out_counts;
    io.d_label_masks = b->d_label_masks;
    io.d_out_pc2 = b->d_out_pc2;
    BatchIO io_score = io;
    if (own_masks) io_score.d_label_masks = ctx->d_score_masks;

    Arena a = ctx->arena;
    a.flags = eff_flags;
    a.eigen_reduction = ctx->conv.eigen_reduction;
    a.fresh_launch = 0;
    // a (half) launch with a cloud of its own configuration takes the kernels' SLOT_CFG variants; any other runs the kernels it always ran
    bool own_half[2] = {false, false};
    for (int i = 0; i < nb; ++i) own_half[i < n_first ? 0 : 1] |= hp[i].cfg_index >= 0;
    a.slot_cfg_launch = own_half[0] ? 1 : 0;
    if (split) {
        // the side stream sees what the caller's stream holds up to here (its inputs, a re-initialisation of the maps on that stream)
        if (!ctx->probe_no_fork) {
            HIPCHK(ctx, hipEventRecord(ctx->half_fork, s));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->half_stream, ctx->half_fork, 0));
        }
        Arena a2 = a; // the words kernels of one launch synchronise through: the second half has its own
        a2.front_sync = a.front_sync2;
        a2.sweep_sync = a.sweep_sync2;
        a2.sweep_rec_clouds = 0; // (one scratch region: the side stream's half keeps k_sweep)
        a2.scan_sync = a.scan_sync2; // (its own region: the halves of consecutive divided batches need not be the same size)
        a2.slot_cfg_launch = own_half[1] ? 1 : 0;
        a.fresh_launch = fresh_half[0] ? 1 : 0;
        a2.fresh_launch = fresh_half[1] ? 1 : 0;
        if (const int rc = fill_fresh(0, n_first, s)) return rc;
        if (const int rc = fill_fresh(n_first, nb, ctx->half_stream)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(dp, hp, sizeof(CloudParams) * n_first, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(dp + n_first, hp + n_first, sizeof(CloudParams) * (nb - n_first), hipMemcpyHostToDevice, ctx->half_stream));
        launch_sequence(ctx, a, dp, score_half[0] ? io_score : io, n_first, max_n[0], s, nullptr, hp[0].slot, false, score_half[0]);
        launch_sequence(ctx, a2, dp + n_first, score_half[1] ? io_score : io, nb - n_first, max_n[1], ctx->half_stream, nullptr, hp[n_first].slot, false, score_half[1]);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, ctx->ring.recorded2(g, ctx->half_stream));
        HIPCHK(ctx, hipEventRecord(ctx->half_done, ctx->half_stream));
        ctx->have_half_event = true;
    } else {
        a.fresh_launch = fresh_half[0] ? 1 : 0;
        if (const int rc = fill_fresh(0, nb, s)) return rc;
        if (const int rc = launch_or_replay(ctx, a, hp, dp, score_half[0] ? io_score : io, nb, max_n[0], s, plan, score_half[0])) return rc;
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, ctx->ring.recorded(g, s));
    HIPCHK(ctx, hipEventRecord(ctx->batch_event, s));
    ctx->last_batch_stream = s;
    ctx->have_batch_event = true;
    if (s != ctx->stream) ctx->map_event_pending = false; // (this stream has waited; later batches anywhere follow batch_event)
    return GG_OK;
}

// The first-call allocation of a many-map call (`who`): a device block, a pinned host block and the events of its parameter ring, and the
// tables the call's kernels read uploaded into the device block (synchronously: they are there before any stream can launch on them).  Not
// while `st` is being captured into a graph: an allocation cannot be captured.  `mem` and `ring` are written when everything is in place:
// nothing of the context changes when this fails (GG_ERR_NOMEM for the two blocks, GG_ERR_HIP for the events and uploads).  `ring` is null
// for a call that runs in another call's frame and takes its ring entries from there: then no events are created.
struct TableUpload {
    size_t offset;
    const void *src;
    size_t bytes;
};
int alloc_call_scratch(gg_context *ctx, const char *who, hipStream_t st, size_t dev_bytes, size_t pinned_bytes, std::initializer_list<TableUpload> tables, CallScratch *mem,
                       ParamRing *ring)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(ctx, GG_ERR_INVALID, who, "the first call allocates its scratch and cannot be captured into a graph");
    (void)hipGetLastError();
    CallScratch m;
    ParamRing r;
    int code = GG_ERR_NOMEM;
    const char *what = "device scratch";
    hipError_t e = m.dev.create(dev_bytes);
    if (e == hipSuccess) {
        what = "pinned parameter ring";
        e = m.pinned.create(pinned_bytes);
    }
    if (e == hipSuccess) code = GG_ERR_HIP;
    if (e == hipSuccess && ring) {
        what = "events";
        e = r.create();
    }
    for (const TableUpload &t : tables)
        if (e == hipSuccess) {
            what = "table upload";
            e = hipMemcpy(m.dev + t.offset, t.src, t.bytes, hipMemcpyHostToDevice);
        }
    if (e != hipSuccess) { // (m and r release what they hold)
        (void)hipGetLastError();
        return fail(ctx, code, (std::string(who) + ": " + what).c_str(), e);
    }
    *mem = std::move(m);
    if (ring) *ring = std::move(r);
    return GG_OK;
}

// GroundGrid::update's host arithmetic (gg_move_map, gg_move_maps): grid_map_core getIndexShiftFromPositionShift -- round half away from
// zero, map frame -> buffer order (sign flip) -- and getPositionShiftFromIndexShift: the position advances by whole cells, not to the
// odometry position
void map_shift(double res, double pos_x, double pos_y, double odom_x, double odom_y, int s[2], double moved[2])
{
    const double odom[2] = {odom_x, odom_y};
    const double pos[2] = {pos_x, pos_y};
    for (int i = 0; i < 2; ++i) {
        const double tmp = (odom[i] - pos[i]) / res;
        s[i] = -(int)(tmp + 0.5 * (tmp > 0 ? 1 : -1));
        moved[i] = pos[i] + (double)(-s[i]) * res;
    }
}

} // namespace

static int rebuild_patch_table(gg_context *ctx, const DevConfig &cfg);

extern "C" {

int gg_abi_version(void) { return GG_ABI_VERSION; }

const char *gg_kernel_name(int k)
{
    static const char *names[GG_NUM_KERNELS] = {"k_classify", "k_scan", "k_scatter", "k_reduce", "k_patch", "k_sweep", "k_label"};
    return (k >= 0 && k < GG_NUM_KERNELS) ? names[k] : "?";
}

void gg_default_config(gg_config *c)
{
    if (!c) return;
    // cfg/GroundGrid.cfg:8-21
    c->point_count_cell_variance_threshold = 10;
    c->max_ring = 1024;
    c->groundpatch_detection_minimum_threshold = 0.01;
    c->distance_factor = 0.0001;
    c->minimum_distance_factor = 0.0005;
    c->miminum_point_height_threshold = 0.3;
    c->minimum_point_height_obstacle_threshold = 0.1;
    c->outlier_tolerance = 0.1;
    c->ground_patch_detection_minimum_point_count_threshold = 0.25;
    c->patch_size_change_distance = 20;
    c->occupied_cells_decrease_factor = 5.0;
    c->occupied_cells_point_count_factor = 20;
    c->min_outlier_detection_ground_confidence = 1.25;
    c->thread_count = 8;
}

void gg_default_geometry(gg_geometry *g)
{
    if (!g) return;
    g->length = 120.0f;                                      // GroundGrid.h:71
    g->resolution = .33f;                                    // GroundGrid.h:70
    g->vertical_point_ang_dist = (float)(0.00174532925 * 2); // GroundSegmentation.h:69
    g->min_dist_squared = 12.0f;                             // GroundSegmentation.h:70
}

int gg_create(const gg_geometry *geom_in, int n_slots, size_t max_points, int device, gg_context **out)
{
    if (!out) return GG_ERR_INVALID;
    *out = nullptr;
    if (n_slots <= 0 || max_points == 0 || max_points > (size_t)1 << 30) return GG_ERR_INVALID;
    gg_geometry geom;
    gg_default_geometry(&geom);
    if (geom_in) {
        if (geom_in->length > 0.f) geom.length = geom_in->length;
        if (geom_in->resolution > 0.f) geom.resolution = geom_in->resolution;
        // the two sensor constants: zero (either sign) selects the reference's value; a negative, infinite or NaN one is an error, not
        // silently the default (a NaN compares false with everything: `> 0` alone would let it through as "zero")
        const float sensor[2] = {geom_in->vertical_point_ang_dist, geom_in->min_dist_squared};
        for (const float v : sensor)
            if (!(v >= 0.f) || isinf(v)) return GG_ERR_GEOMETRY;
        if (geom_in->vertical_point_ang_dist > 0.f) geom.vertical_point_ang_dist = geom_in->vertical_point_ang_dist;
        if (geom_in->min_dist_squared > 0.f) geom.min_dist_squared = geom_in->min_dist_squared;
    }

    // grid_map::GridMap::setGeometry (called at src/GroundGrid.cpp:58)
    const double res = (double)geom.resolution;
    const int n = (int)round((double)geom.length / res);
    // GroundSegmentation::init (src/GroundSegmentation.cpp:38), dimension passed as size_t (Nodelet.cpp:95)
    const size_t dimension = (size_t)geom.length;
    const size_t cellCount = (size_t)roundf((float)dimension / geom.resolution);
    if (n < 8 || (size_t)n != cellCount) return GG_ERR_GEOMETRY;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return GG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GG_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GG_ERR_NO_DEVICE; // this library carries gfx950 code only

    gg_context *ctx = new (std::nothrow) gg_context();
    if (!ctx) return GG_ERR_NOMEM;
    ctx->device = device;
    ctx->geom = geom;
    ctx->n_slots = n_slots;
    ctx->max_points = max_points;
    gg_default_config(&ctx->cfg);
    ctx->pos_x.assign(n_slots, 0.0);
    ctx->no_confidence.assign(n_slots, 0); // layers start as zeros, but only gg_reset_map makes a slot usable
    ctx->fresh.assign(n_slots, 0);
    ctx->fresh_z.assign(n_slots, 0.0f);
    ctx->gp_tainted.assign(n_slots, 0); // (the arena starts zeroed)
    ctx->fresh_enabled = env_int("GG_FRESH_MAPS", 1) != 0;
    ctx->lazy_pending.assign(n_slots, 0);
    ctx->lazy_params.assign(n_slots, CloudParams{});
    ctx->slot_own.assign(n_slots, 0);
    ctx->score_on.assign(n_slots, 0);
    ctx->slot_cfg.assign(n_slots, gg_config{});
    ctx->slot_dev.assign(n_slots, DevConfig{});
    ctx->pos_y.assign(n_slots, 0.0);

#define CREATE_CHK(call)                                             \
    do {                                                             \
        hipError_t e__ = (call);                                     \
        if (e__ != hipSuccess) {                                     \
            fprintf(stderr, "groundgrid_hip: %s failed: %s\n", #call, hipGetErrorString(e__)); \
            gg_destroy(ctx);                                         \
            return e__ == hipErrorOutOfMemory ? GG_ERR_NOMEM : GG_ERR_HIP; \
        }                                                            \
    } while (0)

    CREATE_CHK(hipSetDevice(device));
    CREATE_CHK(ctx->stream.create());
    CREATE_CHK(ctx->h2d_stream.create());
    CREATE_CHK(ctx->d2h_stream.create());
    CREATE_CHK(ctx->half_stream.create());
    CREATE_CHK(ctx->half_fork.create());
    CREATE_CHK(ctx->half_done.create());
    CREATE_CHK(ctx->map_event.create());
    CREATE_CHK(ctx->batch_event.create());
    CREATE_CHK(ctx->gather_event.create());
    CREATE_CHK(ctx->fork_event.create());
    CREATE_CHK(ctx->join_event.create());
    CREATE_CHK(ctx->layers_event.create());
    ctx->graphs_enabled = env_int("GG_GRAPH", 0) != 0; // (1 = one cloud per call replays a captured graph)

    Arena &a = ctx->arena;
    Geometry &g = a.g;
    g.rows = g.cols = n;
    g.C = n * n;
    g.tiles_r = (n + TILE - 1) / TILE;
    g.tiles_c = (n + TILE - 1) / TILE;
    g.T = g.tiles_r * g.tiles_c;
    g.resolution = res;
    g.inv_resolution = 1.0 / res;
    g.length0 = g.length1 = (double)n * res;
    g.half0 = 0.5 * g.length0;
    g.half1 = 0.5 * g.length1;
    g.resolution_f = (float)res;
    g.min_dist_squared = geom.min_dist_squared;
    g.center = n / 2 - 1;
    a.hist_pitch = (g.T + 3) & ~3;
    a.n_slots = n_slots;
    if (g.T > 65535 || (size_t)4 * a.hist_pitch * sizeof(uint32_t) > 150 * 1024) {
        gg_destroy(ctx);
        return GG_ERR_GEOMETRY; // per-wave LDS tile histograms no longer fit
    }
    // points per wavefront chunk of K1 / scatter / K5: the chunk histograms (K1 -> k_scan -> k_scatter) shrink with it, the
    // number of wavefronts per cloud too -- contexts for big batches take 2048 (k_scan 0.18 -> 0.11 ms per 1024 clouds), small
    // ones 1024 (one cloud: 0.56 instead of 0.60 ms)
    a.PW = g.T <= 1024 ? (n_slots >= PW_BIG_CONTEXT_SLOTS ? 2048 : 1024) : 8192;
    a.PW = env_int("GG_PW", a.PW); // (tools, tests: points per wavefront chunk of K1 / scatter / K5)
    if (a.PW < 64 || a.PW % 64 != 0) {
        gg_destroy(ctx);
        return GG_ERR_INVALID;
    }
    a.tune_sweep_waves = env_int("GG_SWEEP_WAVES", 0);
    a.tune_sweep_gpw = env_int("GG_SWEEP_GPW", 0);
    a.tune_sweep_split = env_int("GG_SWEEP_SPLIT", 0);
    a.tune_sweep_pair = env_int("GG_SWEEP_PAIR", 0);
    a.tune_sweep_pair_wgs = env_int("GG_SWEEP_PAIR_WGS", 0);
    a.tune_sweep_pair_waves = env_int("GG_SWEEP_PAIR_WAVES", 0);
    a.tune_front = env_int("GG_FRONT", 0);
    a.tune_k2_per_cloud = env_int("GG_K2_PER_CLOUD", 0);
    a.tune_k2_dense_share = env_int("GG_K2_DENSE_SHARE", 0);
    a.k2_skip = env_int("GG_K2_SKIP", 0);
    make_dev_config(ctx->cfg, a.cfg);

    // R1: expectedPoints (src/GroundSegmentation.cpp:40-46) -- host libm atanf, as in the reference
    ctx->h_expected.resize((size_t)g.C);
    for (size_t i = 0; i < cellCount; ++i)
        for (size_t j = 0; j < cellCount; ++j) {
            const float dist = (float)hypot((double)i - (double)cellCount / 2.0, (double)j - (double)cellCount / 2.0);
            ctx->h_expected[i + j * cellCount] = atanf(1 / dist) / geom.vertical_point_ang_dist;
        }

    ctx->sweep_params = gg::sweep::make_params(n, res, geom.min_dist_squared, ctx->cfg.occupied_cells_decrease_factor);
    if (gg::sweep_lds_bytes(ctx->sweep_params) > 158 * 1024) {
        gg_destroy(ctx);
        return GG_ERR_GEOMETRY; // the sweep's hand-over tables no longer fit in LDS even with one ring group per work-group (n > ~1500)
    }
    std::vector<uint16_t> tile_rank(g.T), rank_tile(g.T);
    {
        std::vector<std::pair<uint32_t, int>> order(g.T);
        for (int tc = 0; tc < g.tiles_c; ++tc)
            for (int tr = 0; tr < g.tiles_r; ++tr) order[tr + tc * g.tiles_r] = {morton2((uint32_t)tr, (uint32_t)tc), tr + tc * g.tiles_r};
        std::sort(order.begin(), order.end());
        for (int r = 0; r < g.T; ++r) {
            rank_tile[r] = (uint16_t)order[r].second;
            tile_rank[order[r].second] = (uint16_t)r;
        }
    }

    // ---- the arena: laid out once (arena_layout.h), counted, allocated, assigned ------------
    std::vector<int> gp_border; // the elements of the cells no sweep visits: ring >= c
    {
        const GpLayout L = make_gp_layout(n);
        for (int col = 0; col < n; ++col)
            for (int row = 0; row < n; ++row)
                if (std::max(std::abs(row - L.c), std::abs(col - L.c)) >= L.c) gp_border.push_back(gp_index(L, row, col));
    }
    const int k2_debug = env_int("GG_K2_DEBUG", 0);
    ArenaShape shape{};
    shape.g = g;
    shape.n_slots = n_slots;
    shape.max_points = max_points;
    shape.PW = a.PW;
    shape.hist_pitch = a.hist_pitch;
    shape.gp_border_n = (int)gp_border.size();
    shape.k2_timing = k2_debug == 9 || k2_debug == 5 || k2_debug == 6;
    shape.sweep_timing = getenv("GG_SWEEP_TIMING") != nullptr;
    shape.pair_timing = getenv("GG_PAIR_TIMING") != nullptr;
    shape.sweep_xchg_entries = gg::sweep_xchg_entries(ctx->sweep_params);
    shape.sweep_pair_rec_floats = gg::sweep_pair_rec_floats(ctx->sweep_params);
    ArenaCounter count;
    lay_out_arena(count, shape, a, *ctx);
    ctx->arena_bytes = count.bytes;
    CREATE_CHK(ctx->d_arena.create(ctx->arena_bytes));
    CREATE_CHK(hipMemsetAsync(ctx->d_arena, 0, ctx->arena_bytes, ctx->stream));
    ArenaAssigner assign{static_cast<char *>(ctx->d_arena.get())};
    lay_out_arena(assign, shape, a, *ctx);
    a.flags = 0;
    a.k2_debug = k2_debug;
    a.k3_debug = env_int("GG_K3_DEBUG", 0);
    a.k5_debug = env_int("GG_K5_DEBUG", 0);
    {
        int row, col;
        if (gp_cell_of(a.gpl, a.gp_fresh_cell, row, col)) { // (cannot happen: sheared position VS - 1 of ring 1 is column n + 125)
            gg_destroy(ctx);
            return GG_ERR_INVALID;
        }
    }
    {
        const uint32_t first_epoch[4] = {0u, 0u, 1u, 0u}; // (the exchange region starts zeroed: tag 0 is never current)
        CREATE_CHK(hipMemcpyAsync(a.sweep_sync, first_epoch, sizeof first_epoch, hipMemcpyHostToDevice, ctx->stream));
        const uint32_t first_epoch2[4] = {0u, 0u, 0x80000001u, 0u}; // (the second set's epochs carry bit 31: k4_sweep.hip)
        CREATE_CHK(hipMemcpyAsync(a.sweep_sync2, first_epoch2, sizeof first_epoch2, hipMemcpyHostToDevice, ctx->stream));
        CREATE_CHK(hipStreamSynchronize(ctx->stream));
    }
    {
        // one word the kernels can reach and the host can read without a copy: a bounded wait that ran out reports here
        CREATE_CHK(ctx->h_dev_error.create(64, hipHostMallocMapped));
        *ctx->h_dev_error = 0u;
        void *dptr = nullptr;
        CREATE_CHK(hipHostGetDevicePointer(&dptr, (void *)ctx->h_dev_error.get(), 0));
        a.dev_error = (uint32_t *)dptr;
    }
    CREATE_CHK(hipMemcpyAsync(const_cast<int *>(a.gp_border), gp_border.data(), gp_border.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    {   // does detect_ground_patches visit a cell of ring >= c?  (rebuild_patch_table's "visited": rows 2 .. 2 (cols / 2) - 3, columns 2 .. rows - 3)
        const int c = n / 2 - 1;
        a.gp_border_patched = 0;
        for (int col = 2; col < n - 2; ++col)
            for (int row = 2; row < 2 * (n / 2) - 2; ++row)
                if (std::max(std::abs(row - c), std::abs(col - c)) >= c) a.gp_border_patched = 1;
    }
    CREATE_CHK(hipStreamSynchronize(ctx->stream));
    if (ctx->d_sweep_dbg) {
        const unsigned long long mode = getenv("GG_SWEEP_DEBUG") ? strtoull(getenv("GG_SWEEP_DEBUG"), nullptr, 0) : 0ull;
        CREATE_CHK(hipStreamSynchronize(ctx->stream)); // (the arena memset above)
        CREATE_CHK(hipMemcpy(ctx->d_sweep_dbg + 63, &mode, 8, hipMemcpyHostToDevice));
    }

    const size_t gp_valid_words = ((size_t)a.gpl.elems + 31) / 32; // one bit per element of the layer
    std::vector<uint32_t> gp_valid(gp_valid_words, 0u);
    for (int col = 0; col < n; ++col)
        for (int row = 0; row < n; ++row) {
            const int e = gp_index(a.gpl, row, col);
            gp_valid[(size_t)e >> 5] |= 1u << (e & 31);
        }
    {
        // The mask only steers the fill of gg_reset_maps, and the padding is never read: every 128-byte line (16 elements) that
        // holds a cell is filled whole.  More than half of the lines with cells are only partly cells (the shear), and a partly
        // written line costs the memory a read-modify-write: 1024 maps take 0.60 ms with the exact mask (1.09 GB), 0.41 ms with
        // whole 64-byte sectors, 0.36 ms with whole lines (1.52 GB, 4.3 TB/s).
        const int group = env_int("GG_FILL_GROUP", 16); // elements; 1 = exact mask (measurement)
        if (group == 8 || group == 16 || group == 32)
            for (size_t w = 0; w < gp_valid_words; ++w) {
                uint32_t v = gp_valid[w], o = 0u;
                for (int b = 0; b < 32; b += group) {
                    const uint32_t gm = (group == 32 ? 0xFFFFFFFFu : ((1u << group) - 1u)) << b;
                    if (v & gm) o |= gm;
                }
                gp_valid[w] = o;
            }
    }
    CREATE_CHK(hipMemcpyAsync(const_cast<uint32_t *>(a.gp_valid), gp_valid.data(), gp_valid_words * 4, hipMemcpyHostToDevice, ctx->stream));
    CREATE_CHK(hipMemcpyAsync(const_cast<float *>(a.expected), ctx->h_expected.data(), (size_t)g.C * 4, hipMemcpyHostToDevice, ctx->stream));
    CREATE_CHK(hipMemcpyAsync(const_cast<uint16_t *>(a.tile_rank), tile_rank.data(), (size_t)g.T * 2, hipMemcpyHostToDevice, ctx->stream));
    CREATE_CHK(hipMemcpyAsync(const_cast<uint16_t *>(a.rank_tile), rank_tile.data(), (size_t)g.T * 2, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> rank_cell0(g.T);
    for (int r = 0; r < g.T; ++r) {
        const int tile = rank_tile[r];
        rank_cell0[r] = (uint32_t)((tile % g.tiles_r) * TILE) | ((uint32_t)((tile / g.tiles_r) * TILE) << 16);
    }
    CREATE_CHK(hipMemcpyAsync(const_cast<uint32_t *>(a.rank_cell0), rank_cell0.data(), (size_t)g.T * 4, hipMemcpyHostToDevice, ctx->stream));
    // The one-map lists of the single-map getters and setters (extract_planes, insert_planes, gg_insert_cloud): entry s = slot s, NOT fresh.
    // Every such caller runs behind own_stream_waits_for_batches' make_real or behind its own call's sweep, so the layer in memory is the map
    std::vector<ExportMap> slot_maps((size_t)n_slots);
    for (int s = 0; s < n_slots; ++s) slot_maps[(size_t)s] = ExportMap{s, 0, 0.0f, 0};
    CREATE_CHK(hipMemcpyAsync(const_cast<ExportMap *>(ctx->d_slot_maps), slot_maps.data(), slot_maps.size() * sizeof(ExportMap), hipMemcpyHostToDevice, ctx->stream));
    CREATE_CHK(hipStreamSynchronize(ctx->stream)); // the host vectors above go out of scope

    CREATE_CHK(ctx->h_params.create(sizeof(CloudParams) * PARAM_RING * n_slots));
    CREATE_CHK(ctx->h_stage_pts.create(max_points * sizeof(gg_point16)));
    CREATE_CHK(ctx->h_stage_labels.create(max_points));
    CREATE_CHK(ctx->h_stage_index.create(max_points * 4));
    CREATE_CHK(ctx->h_stage_counts.create(64));
    CREATE_CHK(ctx->ring.create());
    for (int k = 0; k < GG_ASYNC_DEPTH; ++k) {
        gg_context::AsyncSlot &as = ctx->async_slot[k];
        CREATE_CHK(as.h_pts.create(max_points * sizeof(gg_point16)));
        CREATE_CHK(as.h_counts.create(64 + max_points * 5 + 64)); // (the same block on the host)
        as.h_index = as.h_counts + 16;
        if (hipHostGetDevicePointer((void **)&as.hd_counts, as.h_counts, 0) != hipSuccess) { // (no device view of pinned memory: the results take the copy)
            as.hd_counts = nullptr;
            (void)hipGetLastError();
        }
        CREATE_CHK(as.uploaded.create());
        CREATE_CHK(as.computed.create());
        CREATE_CHK(as.downloaded.create());
    }

    ctx->helper.configure(std::max(1, std::min(env_int("GG_HOST_THREADS", 8), 16)) - 1); // (never more than the usable CPUs - 1: host_helper.h)
    {
        const int rc = rebuild_patch_table(ctx, a.cfg);
        if (rc != GG_OK) {
            gg_destroy(ctx);
            return rc;
        }
    }
    {
        const int rc = gg_reset_maps(ctx, 0, n_slots, 0.0, 0.0, 0.0f, 0, nullptr); // (one strided fill per layer for all slots)
        if (rc != GG_OK) {
            gg_destroy(ctx);
            return rc;
        }
    }
    CREATE_CHK(hipStreamSynchronize(ctx->stream));
#undef CREATE_CHK
    *out = ctx;
    return GG_OK;
}

void gg_destroy(gg_context *ctx)
{
    if (!ctx) return;
    ctx->helper.stop();
    hipSetDevice(ctx->device);
    if (ctx->have_batch_event) hipEventSynchronize(ctx->batch_event);
    if (ctx->half_stream) hipStreamSynchronize(ctx->half_stream);
    if (ctx->h2d_stream) hipStreamSynchronize(ctx->h2d_stream);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->d2h_stream) hipStreamSynchronize(ctx->d2h_stream);
    for (auto &r : ctx->registered) hipHostUnregister(r.first);
    ctx->registered.clear();
    drop_graphs(ctx);
    release_profile_events(ctx);
    delete ctx;
}

// The per-cell constants of detect_ground_patches (gg_internal.h Arena::patch_table), in the reference's own arithmetic: every cell
// used to recompute them for every cloud -- a dozen binary64 operations and the sheared layer index per cell and call, a sixth of
// k_patch's instructions -- although they depend on the cell and the configuration only.
// `cfg`: the configuration the table is for -- the caller commits it to the context only when the table is in place, so that k_patch's
// thresholds and the rest of the path never come from two configurations.
// every batch enqueued so far has finished (what gg_set_config and gg_set_slot_configs wait for before they change what batches read)
static int wait_for_batches_in_flight(gg_context *ctx)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->have_batch_event) HIPCHK(ctx, hipEventSynchronize(ctx->batch_event));
    if (ctx->have_half_event) HIPCHK(ctx, hipEventSynchronize(ctx->half_done));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

static int rebuild_patch_table(gg_context *ctx, const DevConfig &cfg)
{
    const Geometry &g = ctx->arena.g;
    const int rows = g.rows, cols = g.cols;
    std::vector<float> t((size_t)g.C * 4);
    const double res2 = (double)g.resolution_f * (double)g.resolution_f;
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
            float *e = &t[((size_t)i + (size_t)j * rows) * 4];
            const float expected = ctx->h_expected[(size_t)i + (size_t)j * rows];
            // the four quadrants (:325-328) cover rows [2, 2 * (cols / 2) - 2) and cols [2, rows - 2)
            const bool visited = i >= 2 && j >= 2 && !(i >= 2 * (cols / 2) - 2 || j >= rows - 2);
            const double di = (double)i - (double)rows / 2.0, dj = (double)j - (double)cols / 2.0;
            const float sqdist = (float)((di * di + dj * dj) * res2);                          // :332
            const bool near = (double)sqdist <= cfg.patch_size_change_distance_sq;             // :334
            const double S = near ? 3.0 : 5.0;
            const double thr = std::max(floor(cfg.gpd_min_point_count_threshold * S * (double)expected), 3.0); // :364 (an integer-valued double)
            const float thr_f = (float)thr;
            e[0] = expected;
            // (a threshold too large for an exact float -- absurd configurations -- can never be met by a count below 2^24 either)
            e[1] = !visited || !(thr < 16777216.0) ? INFINITY : (near ? -thr_f : thr_f);
            e[2] = (float)std::min(std::max((double)sqdist * cfg.distance_factor_sq, cfg.minimum_distance_factor_sq), cfg.minimum_distance_factor_x10_sq); // :369
            const int gidx = gp_index(ctx->arena.gpl, i, j);
            memcpy(&e[3], &gidx, 4);
        }
    // (batches may be reading the old table: wait for them; gg_set_config is a rare, synchronous call)
    if (const int rc = wait_for_batches_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipMemcpy(const_cast<float4 *>(ctx->arena.patch_table), t.data(), t.size() * 4, hipMemcpyHostToDevice));
    return GG_OK;
}

int gg_set_config(gg_context *ctx, const gg_config *cfg)
{
    if (!ctx || !cfg) return GG_ERR_INVALID;
    // src/GroundSegmentation.cpp:468-471.  Unlike the reference's struct copy this call BLOCKS: it waits for the batches in flight
    // (they read the old table), rebuilds the per-cell table of detect_ground_patches on the host (O(cells)) and uploads it.
    DevConfig dev;
    make_dev_config(*cfg, dev);
    if (const int rc = rebuild_patch_table(ctx, dev)) return rc; // (on failure the context keeps its old configuration AND table)
    ctx->cfg = *cfg;
    ctx->arena.cfg = dev;
    drop_graphs(ctx); // (captured launches carry the old configuration by value)
    return GG_OK;
}

int gg_get_config(const gg_context *ctx, gg_config *cfg)
{
    if (!ctx || !cfg) return GG_ERR_INVALID;
    *cfg = ctx->cfg;
    return GG_OK;
}

// Per-slot configurations.  The context's configuration stays where it was (Arena::cfg and the per-cell table, gg_set_config); a slot
// with its own has its DevConfig in a device table (Arena::slot_cfg, entry = slot) that every launch names and only this call writes, and
// its clouds carry the entry's index (CloudParams::cfg_index).  Launches with such a cloud take the kernels' SLOT_CFG variants.
int gg_set_slot_configs(gg_context *ctx, int n, const int32_t *slots, int first_slot, const gg_config *cfgs)
{
    if (!ctx || n < 0) return fail(ctx, GG_ERR_INVALID, "gg_set_slot_configs: null context or n < 0");
    if (n == 0) return GG_OK;
    if (const int rc = check_slot_list(ctx, "gg_set_slot_configs", n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_slot_cfg && ctx->d_slot_cfg.create(sizeof(DevConfig) * (size_t)ctx->n_slots) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GG_ERR_NOMEM, "gg_set_slot_configs: device table");
    }
    std::vector<char> own = ctx->slot_own;
    std::vector<gg_config> cfg = ctx->slot_cfg;
    std::vector<DevConfig> dev = ctx->slot_dev;
    for (int k = 0; k < n; ++k) {
        const int slot = slot_of(slots, first_slot, k);
        own[slot] = cfgs ? 1 : 0;
        cfg[slot] = cfgs ? cfgs[k] : gg_config{};
        dev[slot] = DevConfig{};
        if (cfgs) make_dev_config(cfgs[k], dev[slot]);
    }
    // (batches in flight read the old table and carry the old indices: they finish first, like gg_set_config's)
    if (const int rc = wait_for_batches_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipMemcpy(ctx->d_slot_cfg, dev.data(), sizeof(DevConfig) * dev.size(), hipMemcpyHostToDevice));
    ctx->slot_own.swap(own);
    ctx->slot_cfg.swap(cfg);
    ctx->slot_dev.swap(dev);
    ctx->arena.slot_cfg = ctx->d_slot_cfg;
    drop_graphs(ctx); // (a captured launch names the kernels and the context configuration it was captured with)
    return GG_OK;
}

int gg_get_slot_config(const gg_context *ctx, int slot, gg_config *cfg, int *own)
{
    if (!ctx || !cfg) return GG_ERR_INVALID;
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    const bool o = ctx->slot_own[slot] != 0;
    *cfg = o ? ctx->slot_cfg[slot] : ctx->cfg;
    if (own) *own = o ? 1 : 0;
    return GG_OK;
}

// ---- evaluator counters (include/groundgrid_hip.h "the score of a labelled cloud", k8_score.hip) ----

int gg_set_score_labels(gg_context *ctx, int n_ids, const int32_t *ids)
{
    if (!ctx || !ids || n_ids < 1 || n_ids > GG_SCORE_MAX_LABELS) return fail(ctx, GG_ERR_INVALID, "gg_set_score_labels: null argument or n_ids outside 1..GG_SCORE_MAX_LABELS");
    std::vector<uint8_t> table(65536, (uint8_t)n_ids); // every id that is not listed: the last bin
    for (int k = 0; k < n_ids; ++k) {
        if (ids[k] < 0 || ids[k] > 65535) return fail(ctx, GG_ERR_INVALID, "gg_set_score_labels: id outside 0..65535");
        if (table[(size_t)ids[k]] != (uint8_t)n_ids) return fail(ctx, GG_ERR_INVALID, "gg_set_score_labels: an id is listed twice");
        table[(size_t)ids[k]] = (uint8_t)k;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t on_off = 65536, scores_off = align_up(on_off + (size_t)ctx->n_slots, 256), scores_bytes = (size_t)ctx->n_slots * SCORE_WORDS * 8;
    const size_t masks_off = align_up(scores_off + scores_bytes, 256);
    if (!ctx->d_score_block) {
        const size_t masks_bytes = (size_t)ctx->n_slots * ((ctx->max_points + 3) / 4) + 64;
        DeviceBlock<uint8_t> block;
        if (block.create(masks_off + masks_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, GG_ERR_NOMEM, "gg_set_score_labels: device block");
        }
        if (hipMemset(block, 0, masks_off) != hipSuccess) { // (every slot off, every counter 0)
            return fail(ctx, GG_ERR_HIP, "gg_set_score_labels: hipMemset");
        }
        ctx->d_score_block = std::move(block);
        uint8_t *base = ctx->d_score_block;
        ctx->score.ring_bin = base;
        ctx->score.slot_on = base + on_off;
        ctx->score.scores = reinterpret_cast<unsigned long long *>(base + scores_off);
        ctx->d_score_masks = base + masks_off;
        ctx->score_masks_bytes = masks_bytes;
    }
    // (batches in flight count into the old bins: they finish first)
    if (const int rc = wait_for_batches_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipMemcpy(const_cast<uint8_t *>(ctx->score.ring_bin), table.data(), table.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemset(ctx->score.scores, 0, scores_bytes));
    ctx->score_n_ids = n_ids;
    return GG_OK;
}

int gg_set_slot_scoring(gg_context *ctx, int n, const int32_t *slots, int first_slot, int enable)
{
    if (!ctx || n < 0) return fail(ctx, GG_ERR_INVALID, "gg_set_slot_scoring: null context or n < 0");
    if (!ctx->score_n_ids) return fail(ctx, GG_ERR_INVALID, "gg_set_slot_scoring: no label list (gg_set_score_labels)");
    if (n == 0) return GG_OK;
    if (const int rc = check_slot_list(ctx, "gg_set_slot_scoring", n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<char> on = ctx->score_on;
    for (int k = 0; k < n; ++k) on[slot_of(slots, first_slot, k)] = enable ? 1 : 0;
    if (const int rc = wait_for_batches_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipMemcpy(const_cast<uint8_t *>(ctx->score.slot_on), on.data(), on.size(), hipMemcpyHostToDevice));
    ctx->score_on.swap(on);
    drop_graphs(ctx); // (a captured launch sequence ends with k_score, or does not)
    return GG_OK;
}

int gg_get_slot_scores(gg_context *ctx, int n, const int32_t *slots, int first_slot, gg_slot_scores *out)
{
    static_assert(sizeof(gg_slot_scores) == (size_t)SCORE_WORDS * 8, "the device keeps a slot's counters in the layout of gg_slot_scores");
    if (!ctx || n < 0 || (!out && n > 0)) return fail(ctx, GG_ERR_INVALID, "gg_get_slot_scores: null argument or n < 0");
    if (!ctx->score_n_ids) return fail(ctx, GG_ERR_INVALID, "gg_get_slot_scores: no label list (gg_set_score_labels)");
    if (n == 0) return GG_OK;
    if (const int rc = check_slot_list(ctx, "gg_get_slot_scores", n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // behind every batch (and second half) enqueued so far -- but no map is read: fresh maps stay as they are
    if (const int rc = own_stream_waits_for_batches(ctx, false)) return rc;
    int lo = ctx->n_slots, hi = 0;
    for (int k = 0; k < n; ++k) {
        const int slot = slot_of(slots, first_slot, k);
        lo = std::min(lo, slot), hi = std::max(hi, slot + 1);
    }
    if (!slots) { // a run of slots: straight into the caller's array
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->score.scores + (size_t)lo * SCORE_WORDS, (size_t)n * sizeof(gg_slot_scores), hipMemcpyDeviceToHost, ctx->stream));
        SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
        return GG_OK;
    }
    std::vector<gg_slot_scores> all((size_t)(hi - lo));
    HIPCHK(ctx, hipMemcpyAsync(all.data(), ctx->score.scores + (size_t)lo * SCORE_WORDS, all.size() * sizeof(gg_slot_scores), hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; ++k) out[k] = all[(size_t)(slots[k] - lo)];
    return GG_OK;
}

int gg_reset_slot_scores(gg_context *ctx, int n, const int32_t *slots, int first_slot)
{
    if (!ctx || n < 0) return fail(ctx, GG_ERR_INVALID, "gg_reset_slot_scores: null context or n < 0");
    if (!ctx->score_n_ids) return fail(ctx, GG_ERR_INVALID, "gg_reset_slot_scores: no label list (gg_set_score_labels)");
    if (n == 0) return GG_OK;
    if (const int rc = check_slot_list(ctx, "gg_reset_slot_scores", n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = wait_for_batches_in_flight(ctx)) return rc;
    if (!slots)
        HIPCHK(ctx, hipMemset(ctx->score.scores + (size_t)first_slot * SCORE_WORDS, 0, (size_t)n * SCORE_WORDS * 8));
    else
        for (int k = 0; k < n; ++k) HIPCHK(ctx, hipMemset(ctx->score.scores + (size_t)slots[k] * SCORE_WORDS, 0, (size_t)SCORE_WORDS * 8));
    return GG_OK;
}

int gg_get_score_kernel_time(gg_context *ctx, double *ms, int64_t *launches, int reset)
{
    if (!ctx) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = drain_profile(ctx)) return rc;
    if (ms) *ms = ctx->k_ms[K_SCORE];
    if (launches) *launches = ctx->k_launches[K_SCORE];
    if (reset) ctx->k_ms[K_SCORE] = 0.0, ctx->k_launches[K_SCORE] = 0;
    return GG_OK;
}

int gg_set_flags(gg_context *ctx, unsigned flags)
{
    if (!ctx) return GG_ERR_INVALID;
    // (leaving GG_FLAG_MINIMAL_LAYERS needs no repair: the next cloud writes all nine layers in the half columns it marks live, and
    // every other column logically holds the reset values anyway -- gg_internal.h tile_live)
    if (flags != ctx->flags) drop_graphs(ctx);
    ctx->flags = flags;
    return GG_OK;
}

int gg_set_conventions(gg_context *ctx, const gg_conventions *conv)
{
    if (!ctx || !conv) return GG_ERR_INVALID;
    if (conv->eigen_reduction != GG_EIGEN_33 && conv->eigen_reduction != GG_EIGEN_34_SSE) return fail(ctx, GG_ERR_INVALID, "eigen_reduction");
    for (int r : conv->reserved)
        if (r != 0) return fail(ctx, GG_ERR_INVALID, "gg_conventions.reserved must be 0");
    ctx->conv = *conv;
    drop_graphs(ctx);
    return GG_OK;
}

int gg_get_conventions(const gg_context *ctx, gg_conventions *conv)
{
    if (!ctx || !conv) return GG_ERR_INVALID;
    *conv = ctx->conv;
    return GG_OK;
}

// host arithmetic only (this file is compiled with -ffp-contract=off: no fused multiply-adds, like the x86-64 reference)
int gg_rotation_from_quaternion(int convention, const double q[4], double R[9])
{
    if (!q || !R) return GG_ERR_INVALID;
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    if (convention == GG_ROT_TF2) { // tf2/LinearMath/Matrix3x3.h setRotation
        const double d = x * x + y * y + z * z + w * w;
        const double s = 2.0 / d;
        const double xs = x * s, ys = y * s, zs = z * s;
        const double wx = w * xs, wy = w * ys, wz = w * zs;
        const double xx = x * xs, xy = x * ys, xz = x * zs;
        const double yy = y * ys, yz = y * zs, zz = z * zs;
        R[0] = 1.0 - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
        R[3] = xy + wz;         R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
        R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.0 - (xx + yy);
    } else if (convention == GG_ROT_KDL) { // orocos_kdl frames.cpp Rotation::Quaternion
        const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
        R[0] = w2 + x2 - y2 - z2;     R[1] = 2 * x * y - 2 * w * z; R[2] = 2 * x * z + 2 * w * y;
        R[3] = 2 * x * y + 2 * w * z; R[4] = w2 - x2 + y2 - z2;     R[5] = 2 * y * z - 2 * w * x;
        R[6] = 2 * x * z - 2 * w * y; R[7] = 2 * y * z + 2 * w * x; R[8] = w2 - x2 - y2 + z2;
    } else {
        return GG_ERR_INVALID;
    }
    return GG_OK;
}

int gg_transform_from_pose(int convention, const double pose7[7], double out12[12])
{
    if (!pose7 || !out12) return GG_ERR_INVALID;
    double R[9];
    const int rc = gg_rotation_from_quaternion(convention, pose7 + 3, R);
    if (rc != GG_OK) return rc;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out12[r * 4 + c] = R[r * 3 + c];
        out12[r * 4 + 3] = pose7[r];
    }
    return GG_OK;
}

int gg_get_size(const gg_context *ctx, int *rows, int *cols)
{
    if (!ctx) return GG_ERR_INVALID;
    if (rows) *rows = ctx->arena.g.rows;
    if (cols) *cols = ctx->arena.g.cols;
    return GG_OK;
}

int gg_get_geometry(const gg_context *ctx, double *resolution, double *length_x, double *length_y)
{
    if (!ctx) return GG_ERR_INVALID;
    if (resolution) *resolution = ctx->arena.g.resolution;
    if (length_x) *length_x = ctx->arena.g.length0;
    if (length_y) *length_y = ctx->arena.g.length1;
    return GG_OK;
}

const char *gg_last_error(const gg_context *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int gg_reset_maps(gg_context *ctx, int first_slot, int n, double pos_x, double pos_y, float odom_z, int persistent_only, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    if (n < 0) return fail(ctx, GG_ERR_CAPACITY, "gg_reset_maps: n < 0");
    if (const int rc = check_slot_list(ctx, "gg_reset_maps", n, nullptr, first_slot)) return rc; // (in front of n == 0: an empty run outside the context is an error too)
    if (n == 0) return GG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = pick_stream(ctx, stream);
    for (int s = first_slot; s < first_slot + n; ++s) ctx->fresh[s] = 0; // (whatever they were: rewritten now)
    // GG_FLAG_CONCURRENT_HALVES: on a caller stream the maps of the upper half of the slots are re-initialised on the side stream, where
    // their batches run -- the caller's stream never has to wait for the second half of the batch before
    const int boundary = (ctx->n_slots + 1) / 2;
    const bool split = halves_enabled(ctx) && st != ctx->stream && st != ctx->half_stream && st != nullptr && first_slot < boundary && first_slot + n > boundary;
    if (const int rc = call_follows_context(ctx, st, split)) return rc; // (on a caller's stream: ordered like a batch there)
    const Arena &a = ctx->arena;
    for (int s = first_slot; s < first_slot + n; ++s) {
        ctx->no_confidence[s] = 1; // groundpatch := 1e-7 everywhere (scrolling keeps that: exposed cells get 0)
        ctx->pos_x[s] = pos_x;
        ctx->pos_y[s] = pos_y;
    }
    // src/GroundGrid.cpp:71-75; the layers filter_cloud adds later (:61-75) start at 0.  The slots' regions are equally
    // spaced, so one strided fill per layer covers all n slots.
    const float init[GG_NUM_LAYERS] = {0.0f, odom_z, (float)0.0000001, (float)100.0, (float)-100.0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto fill = [&](int first, int count, hipStream_t on) {
        if (count <= 0) return;
        if (!persistent_only) {
            for (int s = first; s < first + count; ++s) ctx->lazy_pending[s] = 0;
            launch_fill_percall(a, first, count, init, on);
            // these are GroundGrid's initial values, not filter_cloud's per-call reset values: the next cloud rewrites every tile
            launch_fill_bytes((uint8_t *)(a.tile_live + (size_t)first * a.tile_live_stride), (size_t)count * a.tile_live_stride * 4, 0xFF, on);
        }
        if (ctx->fresh_enabled) { // the interior stays unwritten: the next batch's sweep rewrites it anyway (make_real() for everybody else)
            // ... unless a slot's memory may hold sign bits from outside the path (gp_tainted): those runs of slots get the real fill, once
            for (int s = first; s < first + count;) {
                if (!ctx->gp_tainted[s]) {
                    ++s;
                    continue;
                }
                int e = s + 1;
                while (e < first + count && ctx->gp_tainted[e]) ++e;
                launch_fill2_strided(gp2_ptr(a, s), (size_t)a.gpl.elems, a.gp2_stride, e - s, init[GG_LAYER_GROUND], init[GG_LAYER_GROUNDPATCH], a.gp_valid, on);
                for (int k = s; k < e; ++k) ctx->gp_tainted[k] = 0;
                s = e;
            }
            launch_reset_fresh(a, first, count, init[GG_LAYER_GROUND], init[GG_LAYER_GROUNDPATCH], on);
            for (int s = first; s < first + count; ++s) ctx->fresh[s] = 1, ctx->fresh_z[s] = odom_z;
        } else {
            launch_fill2_strided(gp2_ptr(a, first), (size_t)a.gpl.elems, a.gp2_stride, count, init[GG_LAYER_GROUND], init[GG_LAYER_GROUNDPATCH], a.gp_valid, on);
            for (int s = first; s < first + count; ++s) ctx->gp_tainted[s] = 0;
        }
    };
    if (split) {
        if (!ctx->probe_no_fork) {
            HIPCHK(ctx, hipEventRecord(ctx->half_fork, st));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->half_stream, ctx->half_fork, 0));
        }
        fill(first_slot, boundary - first_slot, st);
        fill(boundary, first_slot + n - boundary, ctx->half_stream);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ctx->half_done, ctx->half_stream));
        ctx->have_half_event = true;
    } else {
        fill(first_slot, n, st);
        HIPCHK(ctx, hipGetLastError());
    }
    return call_recorded(ctx, st, false);
}

int gg_reset_map(gg_context *ctx, int slot, double pos_x, double pos_y, float odom_z)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    return gg_reset_maps(ctx, slot, 1, pos_x, pos_y, odom_z, 0, nullptr);
}

int gg_set_map_position(gg_context *ctx, int slot, double pos_x, double pos_y)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    ctx->pos_x[slot] = pos_x;
    ctx->pos_y[slot] = pos_y;
    return GG_OK;
}

int gg_move_map(gg_context *ctx, int slot, double odom_x, double odom_y, const double base_plane[4], int shift_out[2])
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!base_plane) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int s[2];
    double moved[2];
    map_shift(ctx->arena.g.resolution, ctx->pos_x[slot], ctx->pos_y[slot], odom_x, odom_y, s, moved);
    if (shift_out) {
        shift_out[0] = s[0];
        shift_out[1] = s[1];
    }
    if (s[0] == 0 && s[1] == 0) return GG_OK; // src/GroundGrid.cpp:135-137
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    ctx->pos_x[slot] = moved[0];
    ctx->pos_y[slot] = moved[1];
    launch_scroll(ctx->arena, slot, reinterpret_cast<float2 *>(ctx->d_scroll_scratch), s[0], s[1], ctx->pos_x[slot], ctx->pos_y[slot], base_plane, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return own_stream_mutated_map(ctx);
}

// gg_move_maps' device block and pinned parameter ring, at its first call (alloc_call_scratch: nothing of the context changes when it fails)
static int ensure_move_scratch(gg_context *ctx, hipStream_t st)
{
    if (ctx->move_mem.dev) return GG_OK;
    const Arena &a = ctx->arena;
    const size_t row = (size_t)a.g.C * sizeof(float2);
    // scratch rows: one per slot, at most 256 MB (at least 2: the two halves of a divided call each need one)
    const int cap = (int)std::max<size_t>(2, std::min<size_t>((size_t)ctx->n_slots, ((size_t)256 << 20) / row));
    const size_t ring_bytes = (size_t)PARAM_RING * ctx->n_slots * sizeof(MoveParams);
    const size_t o_cells = 0;
    const size_t o_params = align_up(o_cells + (size_t)a.g.C * sizeof(int2), 256);
    const size_t o_scratch = align_up(o_params + ring_bytes, 256);
    std::vector<int2> cells;
    cells.reserve((size_t)a.g.C);
    for (int e = 0; e < a.gpl.elems; ++e) {
        int r, c;
        if (gp_cell_of(a.gpl, e, r, c)) cells.push_back(make_int2(e, r | (c << 16)));
    }
    if ((int)cells.size() != a.g.C) return fail(ctx, GG_ERR_GEOMETRY, "gg_move_maps: the layer's cell elements do not cover the map");
    if (const int rc = alloc_call_scratch(ctx, "gg_move_maps", st, o_scratch + (size_t)cap * row, ring_bytes, {{o_cells, cells.data(), cells.size() * sizeof(int2)}},
                                          &ctx->move_mem, &ctx->move_ring))
        return rc;
    char *block = ctx->move_mem.dev;
    ctx->d_move_cells = (const int2 *)(block + o_cells);
    ctx->d_move_params = (MoveParams *)(block + o_params);
    ctx->d_move_scratch = (float2 *)(block + o_scratch);
    ctx->h_move_params = (MoveParams *)ctx->move_mem.pinned.get();
    ctx->move_cap = cap;
    return GG_OK;
}

int gg_move_maps(gg_context *ctx, int n, const int32_t *slots, int first_slot, const double *odom_xy, const double *base_planes, int32_t *shifts,
                 void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    if (n < 0) return fail(ctx, GG_ERR_INVALID, "gg_move_maps: n < 0");
    if (n == 0) return GG_OK;
    if (!odom_xy || !base_planes) return fail(ctx, GG_ERR_INVALID, "gg_move_maps: odom_xy and base_planes are required");
    if (n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, "gg_move_maps: more maps than the context has");
    // (distinct and in range: two scrolls of one map in one launch would race.  The check above stays in front: a list longer than the context
    // has a duplicate by necessity, and is GG_ERR_CAPACITY all the same)
    if (const int rc = check_slot_list(ctx, "gg_move_maps", n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = pick_stream(ctx, stream);
    const Arena &a = ctx->arena;
    // the shift and the position after the move of every map, as gg_move_map computes them; maps with a zero shift are not touched (:135-137)
    std::vector<int> sh((size_t)2 * n);
    std::vector<double> moved((size_t)2 * n);
    std::vector<int> order; // the maps that move: those of the lower half of the slots first when the call runs as two halves
    order.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int slot = slot_of(slots, first_slot, i);
        map_shift(a.g.resolution, ctx->pos_x[slot], ctx->pos_y[slot], odom_xy[2 * i], odom_xy[2 * i + 1], &sh[(size_t)2 * i], &moved[(size_t)2 * i]);
        if (sh[(size_t)2 * i] != 0 || sh[(size_t)2 * i + 1] != 0) order.push_back(i);
    }
    if (!order.empty()) {
        if (const int rc = ensure_move_scratch(ctx, st)) return rc;
        // GG_FLAG_CONCURRENT_HALVES: on a caller stream the maps of the upper half of the slots scroll on the side stream, where their
        // batches run (as gg_reset_maps divides its fills): a loop of moves and batches on one stream keeps both halves concurrent
        std::stable_partition(order.begin(), order.end(), [&](int i) { return !second_half_slot(ctx, slot_of(slots, first_slot, i)); });
        int n_lo = 0;
        while (n_lo < (int)order.size() && !second_half_slot(ctx, slot_of(slots, first_slot, order[(size_t)n_lo]))) ++n_lo;
        const int nm = (int)order.size();
        const bool split = halves_enabled(ctx) && st != ctx->stream && st != ctx->half_stream && st != nullptr && n_lo > 0 && n_lo < nm;
        // parameter ring slot (the pinned entries are rewritten only when the copy that read them last has run)
        int g;
        HIPCHK(ctx, ctx->move_ring.acquire(&g));
        MoveParams *hp = ctx->h_move_params + (size_t)g * ctx->n_slots;
        MoveParams *dp = ctx->d_move_params + (size_t)g * ctx->n_slots;
        for (int k = 0; k < nm; ++k) {
            const int i = order[(size_t)k], slot = slot_of(slots, first_slot, i);
            MoveParams &p = hp[k];
            p.sp = make_scroll_params(a, sh[(size_t)2 * i], sh[(size_t)2 * i + 1], moved[(size_t)2 * i], moved[(size_t)2 * i + 1], base_planes + (size_t)4 * i);
            p.slot = slot;
            p.fresh = ctx->fresh[slot] ? 1 : 0;
            p.fresh_z = ctx->fresh_z[slot];
        }
        if (const int rc = call_follows_context(ctx, st, split)) return rc; // (ordered like gg_reset_maps on `st`)
        HIPCHK(ctx, hipMemcpyAsync(dp, hp, sizeof(MoveParams) * nm, hipMemcpyHostToDevice, st));
        // chunks of at most `per` maps through the scratch rows [row0, row0 + per): consecutive chunks on one stream reuse them in order
        auto run = [&](int lo, int hi, int row0, int per, hipStream_t on) {
            if (ctx->move_chunk_tune > 0) per = std::min(per, ctx->move_chunk_tune);
            for (int k = lo; k < hi; k += per)
                launch_scroll_batch(a, ctx->d_move_cells, dp + k, std::min(per, hi - k), ctx->d_move_scratch + (size_t)row0 * a.g.C, on);
        };
        if (split) { // (the two halves scroll through disjoint scratch rows: they run side by side)
            HIPCHK(ctx, hipEventRecord(ctx->half_fork, st)); // (behind the parameter upload, which the side stream reads too)
            HIPCHK(ctx, hipStreamWaitEvent(ctx->half_stream, ctx->half_fork, 0));
            const int half = ctx->move_cap / 2;
            run(0, n_lo, 0, half, st);
            run(n_lo, nm, half, half, ctx->half_stream);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, ctx->move_ring.recorded2(g, ctx->half_stream));
            HIPCHK(ctx, hipEventRecord(ctx->half_done, ctx->half_stream));
            ctx->have_half_event = true;
        } else {
            run(0, nm, 0, ctx->move_cap, st);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, ctx->move_ring.recorded(g, st));
        if (const int rc = call_recorded(ctx, st, false)) return rc;
        // every enqueue succeeded: the moved maps are at their new positions, and real (the scroll wrote every cell); no_confidence stays
        for (int i : order) {
            const int slot = slot_of(slots, first_slot, i);
            ctx->pos_x[slot] = moved[(size_t)2 * i];
            ctx->pos_y[slot] = moved[(size_t)2 * i + 1];
            ctx->fresh[slot] = 0;
        }
    }
    if (shifts)
        for (int k = 0; k < 2 * n; ++k) shifts[k] = sh[(size_t)k];
    return GG_OK;
}

// gg_export_layers' and gg_import_layers' device block and pinned rings, at the first call of either (alloc_call_scratch: nothing of the
// context changes when it fails)
static int ensure_export_scratch(gg_context *ctx, const char *who, hipStream_t st)
{
    if (ctx->export_mem.dev) return GG_OK;
    const Arena &a = ctx->arena;
    const int C = a.g.C;
    const int br = (a.g.rows + EXPORT_TILE - 1) / EXPORT_TILE, bc = (a.g.cols + EXPORT_TILE - 1) / EXPORT_TILE;
    // the export table: every block's cells in the order of their elements in the sheared layer
    std::vector<uint32_t> off((size_t)br * bc + 1, 0u), elem;
    std::vector<uint16_t> cell;
    elem.reserve((size_t)C);
    cell.reserve((size_t)C);
    std::vector<std::pair<uint32_t, uint16_t>> blk;
    for (int b = 0; b < br * bc; ++b) {
        const int r0 = (b % br) * EXPORT_TILE, c0 = (b / br) * EXPORT_TILE;
        blk.clear();
        for (int ci = 0; ci < EXPORT_TILE && c0 + ci < a.g.cols; ++ci)
            for (int ri = 0; ri < EXPORT_TILE && r0 + ri < a.g.rows; ++ri) blk.emplace_back((uint32_t)gp_idx(a, r0 + ri, c0 + ci), (uint16_t)(ri | (ci << 6)));
        std::sort(blk.begin(), blk.end());
        for (const auto &e : blk) {
            if (e.first >= (uint32_t)a.gpl.elems) return fail(ctx, GG_ERR_GEOMETRY, who, "a cell's element lies outside the layer");
            elem.push_back(e.first);
            cell.push_back(e.second);
        }
        off[(size_t)b + 1] = (uint32_t)elem.size();
    }
    // both blocks are carved in one order, every part aligned to 256 bytes; a ring table has a part of the same size in either
    size_t dev_end = 0, pinned_end = 0;
    const auto take = [](size_t &end, size_t bytes) {
        const size_t at = align_up(end, 256);
        end = at + bytes;
        return at;
    };
    const auto ring_part = [&](size_t per_entry, size_t elem_bytes) {
        const size_t bytes = PARAM_RING * per_entry * elem_bytes;
        return RingPart{take(dev_end, bytes), take(pinned_end, bytes), per_entry};
    };
    const size_t slots = (size_t)ctx->n_slots;
    const size_t o_off = take(dev_end, off.size() * sizeof(uint32_t));
    const size_t o_elem = take(dev_end, elem.size() * sizeof(uint32_t));
    const size_t o_cell = take(dev_end, cell.size() * sizeof(uint16_t));
    const RingPart maps = ring_part(slots, sizeof(ExportMap)), lazy = ring_part(slots, sizeof(CloudParams));
    // (gg_export_images: the partial bounds of either variant's bounds launch, per ring entry)
    const int parts_cap = std::max(image_parts(a.g, 0), image_parts(a.g, 1));
    const size_t o_partials = take(dev_end, PARAM_RING * slots * GG_NUM_LAYERS * (size_t)parts_cap * 2 * sizeof(float));
    // (the plane calls' tables, in the order the calls were added; between them the partial results of gg_match_planes' two launches)
    const RingPart shifts = ring_part(slots, sizeof(int2)), starts = ring_part(slots, sizeof(int32_t)), pivots = ring_part(slots, sizeof(int2));
    const RingPart rotations = ring_part(MATCH_MAX_ROTATIONS, sizeof(int2));
    const size_t o_match = take(dev_end, PARAM_RING * slots * MATCH_MAX_ROTATIONS * sizeof(MatchPartial));
    const RingPart footprint = ring_part(FOOTPRINT_TABLE, sizeof(uint32_t)), moves = ring_part(HEADINGS_TABLE, sizeof(uint32_t)), poses = ring_part(slots, sizeof(int2));
    const RingPart rollout_starts = ring_part(3 * slots, sizeof(int32_t));
    if (const int rc = alloc_call_scratch(ctx, who, st, dev_end, pinned_end,
                                          {{o_off, off.data(), off.size() * sizeof(uint32_t)}, {o_elem, elem.data(), elem.size() * sizeof(uint32_t)}, {o_cell, cell.data(), cell.size() * sizeof(uint16_t)}},
                                          &ctx->export_mem, &ctx->export_ring))
        return rc;
    const CallScratch &m = ctx->export_mem;
    ctx->d_export_off = (const uint32_t *)(m.dev + o_off);
    ctx->d_export_elem = (const uint32_t *)(m.dev + o_elem);
    ctx->d_export_cell = (const uint16_t *)(m.dev + o_cell);
    ctx->d_export_maps = (ExportMap *)(m.dev + maps.dev);
    ctx->h_export_maps = (ExportMap *)(m.pinned + maps.pinned);
    ctx->d_export_lazy = (CloudParams *)(m.dev + lazy.dev);
    ctx->h_export_lazy = (CloudParams *)(m.pinned + lazy.pinned);
    ctx->d_image_partials = (float *)(m.dev + o_partials);
    ctx->image_parts_cap = parts_cap;
    ctx->d_match_partials = (MatchPartial *)(m.dev + o_match);
    ctx->ring_shifts.bind(m, shifts);
    ctx->ring_starts.bind(m, starts);
    ctx->ring_pivots.bind(m, pivots);
    ctx->ring_rotations.bind(m, rotations);
    ctx->ring_footprint.bind(m, footprint);
    ctx->ring_moves.bind(m, moves);
    ctx->ring_poses.bind(m, poses);
    ctx->ring_rollout_starts.bind(m, rollout_starts);
    return GG_OK;
}

// The frame of the many-map calls that read or write layers (gg_export_layers, gg_import_layers, gg_export_images), on the shared table,
// rings and events.  map_call_begin: the slot list is checked, the ring entry `g` taken, the listed maps' entries filled and uploaded, `st`
// ordered behind the context, and -- lazy_wanted -- the three lazily kept layers computed for the listed maps that still miss them, in one
// launch.  The caller enqueues its kernels on f.st with f.dm, then map_call_end: the ring entry and the call are recorded.  Host-side flags
// are committed by the caller behind that, when every launch has been enqueued.
struct MapCall {
    hipStream_t st = nullptr;
    int g = 0;
    ExportMap *hm = nullptr, *dm = nullptr;
    CloudParams *hl = nullptr;
    int n_lazy = 0; // hl[0 .. n_lazy): the maps whose lazily kept layers the call computed
};
static int map_call_begin(gg_context *ctx, const char *who, int n, const int32_t *slots, int first_slot, void *stream, bool lazy_wanted, MapCall *f)
{
    if (const int rc = check_slot_list(ctx, who, n, slots, first_slot)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    f->st = pick_stream(ctx, stream);
    if (const int rc = ensure_export_scratch(ctx, who, f->st)) return rc;
    // ring entry (the pinned tables are rewritten only when the copies that read them last have run)
    HIPCHK(ctx, ctx->export_ring.acquire(&f->g));
    f->hm = ctx->h_export_maps + (size_t)f->g * ctx->n_slots;
    f->dm = ctx->d_export_maps + (size_t)f->g * ctx->n_slots;
    f->hl = ctx->h_export_lazy + (size_t)f->g * ctx->n_slots;
    CloudParams *dl = ctx->d_export_lazy + (size_t)f->g * ctx->n_slots;
    f->n_lazy = 0;
    for (int i = 0; i < n; ++i) {
        const int slot = slot_of(slots, first_slot, i);
        f->hm[i].slot = slot;
        // (export, images: a fresh map stays fresh: its planes are the reset's constants.  import: with ground / groundpatch named, the kernel
        // writes the whole pair: no fill)
        f->hm[i].fresh = ctx->fresh[slot] ? 1 : 0;
        f->hm[i].fresh_z = ctx->fresh_z[slot];
        f->hm[i].reserved = 0;
        if (lazy_wanted && ctx->lazy_pending[slot]) f->hl[f->n_lazy++] = ctx->lazy_params[slot];
    }
    // `st` follows every earlier map mutation, batch, export and import of the context, and both halves of a divided batch: the call reads
    // (writes) maps of either
    if (const int rc = call_follows_context(ctx, f->st, false)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(f->dm, f->hm, sizeof(ExportMap) * n, hipMemcpyHostToDevice, f->st));
    if (f->n_lazy) { // one launch
        HIPCHK(ctx, hipMemcpyAsync(dl, f->hl, sizeof(CloudParams) * f->n_lazy, hipMemcpyHostToDevice, f->st));
        launch_reduce_lazy_batch(ctx->arena, dl, f->n_lazy, f->st);
    }
    return GG_OK;
}
static int map_call_end(gg_context *ctx, const MapCall &f)
{
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, ctx->export_ring.recorded(f.g, f.st));
    // whatever reads or writes one of these maps next on another stream waits for the call (and for the lazily kept layers it computed)
    return call_recorded(ctx, f.st, true);
}

extern "C++" { // (templates, amid the extern "C" of the ABI)
// A table of the call's ring entry (the entry is the call's own from map_call_begin on): ring_entry() is where the host fills it, and
// ring_upload() enqueues the copy of its first `count` elements on f.st and returns where the kernels read them -- null when the copy
// could not be enqueued, and the context then holds the error
template <typename T>
static T *ring_entry(const RingTable<T> &t, const MapCall &f)
{
    return t.host + (size_t)f.g * t.per_entry;
}
template <typename T>
static const T *ring_upload(gg_context *ctx, const RingTable<T> &t, const MapCall &f, int count)
{
    const size_t at = (size_t)f.g * t.per_entry;
    const hipError_t e = hipMemcpyAsync(t.dev + at, t.host + at, sizeof(T) * count, hipMemcpyHostToDevice, f.st);
    if (e == hipSuccess) return t.dev + at;
    fail(ctx, GG_ERR_HIP, "hipMemcpyAsync of a ring table", e);
    return nullptr;
}

// The plane calls' overlap test (plane_args.h first_overlap): no output may share a byte with an input or another output.  The ranges run
// from a buffer's first word to the last cell of its last plane, a call lists them in the order of its header, and the first pair of that
// order is the one named
template <size_t N>
static int check_no_overlap(gg_context *ctx, const char *who, const BufferRange (&ranges)[N])
{
    const std::pair<int, int> hit = first_overlap(ranges, (int)N);
    if (hit.first < 0) return GG_OK;
    return fail(ctx, GG_ERR_INVALID, who, (std::string(ranges[hit.first].name) + " and " + ranges[hit.second].name + " overlap").c_str());
}
} // extern "C++"

// gg_export_layers and gg_import_layers, its inverse, are one call in two directions; `d_planes` is the destination of the one and the
// source of the other.
static int transfer_layers(gg_context *ctx, bool import, int n, const int32_t *slots, int first_slot, unsigned layer_mask, int order, const float *d_planes,
                           size_t plane_stride, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = import ? "gg_import_layers" : "gg_export_layers";
    if (n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (n == 0) return GG_OK;
    if (layer_mask == 0u || (layer_mask >> GG_NUM_LAYERS) != 0u) return fail(ctx, GG_ERR_INVALID, who, "layer_mask");
    if (order != GG_PLANES_COLMAJOR && order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (!d_planes) return fail(ctx, GG_ERR_INVALID, who, import ? "d_src is null" : "d_dst is null");
    if (plane_stride < (size_t)ctx->arena.g.C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    const unsigned gp_mask = layer_mask & ((1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH));
    const unsigned percall_mask = layer_mask & ~gp_mask;
    const unsigned lazy_mask = LAZY_LAYERS;
    // Which listed maps get the three layers GG_FLAG_MINIMAL_LAYERS left out computed first, where they still miss them:
    // export: those whose lazily kept layers the mask names -- exactly the exported slots that still miss them.
    // import: the import makes all nine per-call layers of a map dense, after which the three lazily kept ones can no longer be computed into
    // the half columns their cloud wrote: a listed map that still misses them gets them first -- unless all three are imported anyway
    const bool lazy_first = percall_mask != 0u && (layer_mask & lazy_mask) != lazy_mask;
    const bool lazy_wanted = import ? lazy_first : (layer_mask & lazy_mask) != 0u;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, slots, first_slot, stream, lazy_wanted, &f)) return rc;
    const PlaneArgs x = fill_plane_args(ctx, f.dm, layer_mask, order, const_cast<float *>(d_planes), plane_stride); // (the import only reads them)
    if (import) launch_import(ctx->arena, x, n, ctx->import_variant, f.st);
    else launch_export(ctx->arena, x, n, ctx->export_variant, f.st);
    if (const int rc = map_call_end(ctx, f)) return rc;
    if (!import) {
        for (int i = 0; i < f.n_lazy; ++i) ctx->lazy_pending[f.hl[i].slot] = 0;
        return GG_OK;
    }
    // import: every launch is enqueued: the listed maps' flags follow (no other map's change)
    for (int i = 0; i < n; ++i) {
        const int slot = slot_of(slots, first_slot, i);
        if (gp_mask) ctx->fresh[slot] = 0; // (the kernel wrote the pair of every cell)
        if (layer_mask & (1u << GG_LAYER_GROUNDPATCH)) ctx->no_confidence[slot] = 0, ctx->gp_tainted[slot] = 1;
        if (percall_mask) ctx->lazy_pending[slot] = 0; // (computed above, or all three imported)
    }
    return GG_OK;
}

int gg_export_layers(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned layer_mask, int order, float *d_dst, size_t plane_stride,
                     void *stream)
{
    return transfer_layers(ctx, false, n, slots, first_slot, layer_mask, order, d_dst, plane_stride, stream);
}

int gg_import_layers(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned layer_mask, int order, const float *d_src,
                     size_t plane_stride, void *stream)
{
    return transfer_layers(ctx, true, n, slots, first_slot, layer_mask, order, d_src, plane_stride, stream);
}

// The slope, step and normal planes of many maps (k14_slopes.hip), in the frame of the export with its checks in its order: stateless, nothing
// is synchronised, no map is filled, the lazily kept layers stay pending and no host flag is committed.
int gg_export_slopes(gg_context *ctx, int n, const int32_t *slots, int first_slot, unsigned channel_mask, int order, float *d_dst, size_t plane_stride,
                     void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_export_slopes";
    if (n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (n == 0) return GG_OK;
    if (channel_mask == 0u || (channel_mask >> GG_NUM_SLOPE_CHANNELS) != 0u) return fail(ctx, GG_ERR_INVALID, who, "channel_mask");
    if (order != GG_PLANES_COLMAJOR && order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (!d_dst) return fail(ctx, GG_ERR_INVALID, who, "d_dst is null");
    if (plane_stride < (size_t)ctx->arena.g.C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, slots, first_slot, stream, false, &f)) return rc;
    launch_slopes(ctx->arena, fill_plane_args(ctx, f.dm, channel_mask, order, d_dst, plane_stride), n, ctx->slopes_variant, f.st);
    return map_call_end(ctx, f);
}

// The u8 layer images and the terrain images of many maps (k11_images.hip), in the frame of the export: nothing is synchronised, no map is
// filled, and the lazily kept layers are computed only where the mask names one of them (the terrain image reads none).
int gg_export_images(gg_context *ctx, const gg_image_export *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_export_images";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_image_export");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    if ((x->layer_mask >> GG_NUM_LAYERS) != 0u) return fail(ctx, GG_ERR_INVALID, who, "layer_mask");
    if (x->layer_mask && !x->d_images) return fail(ctx, GG_ERR_INVALID, who, "d_images is null");
    if (!x->layer_mask && !x->d_terrain) return fail(ctx, GG_ERR_INVALID, who, "neither a layer nor the terrain image is asked for");
    if (x->layer_mask && x->image_stride < C) return fail(ctx, GG_ERR_INVALID, who, "image_stride is smaller than rows * cols");
    if (x->d_terrain && x->terrain_stride < 3 * C) return fail(ctx, GG_ERR_INVALID, who, "terrain_stride is smaller than 3 * rows * cols");
    if (x->d_terrain && x->terrain_layout != GG_TERRAIN_HWC && x->terrain_layout != GG_TERRAIN_CHW) return fail(ctx, GG_ERR_INVALID, who, "terrain_layout");
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, x->n, x->slots, x->first_slot, stream, (x->layer_mask & LAZY_LAYERS) != 0u, &f)) return rc;
    const PlaneArgs table = fill_plane_args(ctx, f.dm, x->layer_mask, GG_PLANES_ROWMAJOR, nullptr, 0);
    ImageArgs im;
    im.maps = f.dm;
    im.block_off = table.block_off;
    im.elem = table.elem;
    im.cell = table.cell;
    im.blocks_r = table.blocks_r;
    im.blocks_c = table.blocks_c;
    im.mask = x->layer_mask;
    im.n_planes = table.n_planes;
    im.images = x->d_images;
    im.image_stride = x->image_stride;
    im.partials = ctx->d_image_partials + (size_t)f.g * ctx->n_slots * GG_NUM_LAYERS * (size_t)ctx->image_parts_cap * 2;
    im.n_parts = image_parts(ctx->arena.g, ctx->images_variant);
    im.bounds = x->d_bounds;
    im.terrain = x->d_terrain;
    im.terrain_stride = x->terrain_stride;
    im.terrain_layout = x->terrain_layout;
    launch_images(ctx->arena, im, x->n, ctx->images_variant, f.st);
    if (const int rc = map_call_end(ctx, f)) return rc;
    for (int i = 0; i < f.n_lazy; ++i) ctx->lazy_pending[f.hl[i].slot] = 0;
    return GG_OK;
}

// gg_split_clouds' and gg_rasterize_clouds' device block and pinned records, at the first call of either (alloc_call_scratch: nothing of the
// context changes when it fails)
static int ensure_split_scratch(gg_context *ctx, const char *who, hipStream_t st)
{
    if (ctx->split_mem.dev) return GG_OK;
    const size_t ring = (size_t)PARAM_RING * ctx->n_slots;
    const size_t o_counts = align_up(ring * sizeof(SplitCloud), 256);
    const size_t n_pairs = ring * (size_t)std::max(ctx->arena.NCH, 1);
    if (const int rc = alloc_call_scratch(ctx, who, st, o_counts + n_pairs * sizeof(uint2), ring * sizeof(SplitCloud), {}, &ctx->split_mem, nullptr)) return rc;
    ctx->d_split_clouds = (SplitCloud *)ctx->split_mem.dev.get();
    ctx->d_split_counts = (uint2 *)(ctx->split_mem.dev + o_counts);
    ctx->h_split_clouds = (SplitCloud *)ctx->split_mem.pinned.get();
    return GG_OK;
}

// What gg_split_clouds and gg_rasterize_clouds take in: the leading members of gg_cloud_split and gg_cloud_raster
struct LabelledClouds {
    int n, first_slot;
    const int32_t *slots;
    int point_format;
    const void *d_points;
    size_t cloud_stride;
    const int32_t *n_points;
    const double *transforms;
    const uint8_t *d_labels, *d_label_masks;
    const float *origins = nullptr; // gg_visibility_clouds alone: host [n][3], the sensor in the map frame
};

// Their frame, the export's: the arguments are checked before anything is touched (in.n > 0), then the call's ring entry is taken, `f->st`
// ordered behind the context, one SplitCloud per cloud uploaded and *cl filled.  The caller enqueues its kernels on f->st, then map_call_end.
static int labelled_clouds_begin(gg_context *ctx, const char *who, const LabelledClouds &in, void *stream, MapCall *f, CloudArgs *cl,
                                 int (*ensure_more)(gg_context *, const char *, hipStream_t) = nullptr)
{
    if (!in.d_points || !in.n_points) return fail(ctx, GG_ERR_INVALID, who, "d_points and n_points are required");
    if (in.point_format != GG_POINT32 && in.point_format != GG_POINT16) return fail(ctx, GG_ERR_INVALID, who, "point_format");
    if ((in.d_labels != nullptr) == (in.d_label_masks != nullptr)) return fail(ctx, GG_ERR_INVALID, who, "exactly one of d_labels and d_label_masks");
    if (in.d_label_masks && in.cloud_stride % 4 != 0) return fail(ctx, GG_ERR_INVALID, who, "d_label_masks needs a cloud_stride that is a multiple of 4");
    if (in.cloud_stride > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, who, "cloud_stride is larger than max_points");
    if (const int rc = check_slot_list(ctx, who, in.n, in.slots, in.first_slot)) return rc;
    int max_n = 0;
    for (int i = 0; i < in.n; ++i) {
        if (in.n_points[i] < 0) return fail(ctx, GG_ERR_INVALID, who, "n_points[i] < 0");
        if ((size_t)in.n_points[i] > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, who, "a cloud is larger than max_points");
        if ((size_t)in.n_points[i] > in.cloud_stride) return fail(ctx, GG_ERR_INVALID, who, "n_points[i] is larger than cloud_stride");
        max_n = std::max(max_n, (int)in.n_points[i]);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = ensure_split_scratch(ctx, who, pick_stream(ctx, stream))) return rc;
    if (ensure_more) // (a call with scratch of its own: checked arguments first, and no ring entry taken yet)
        if (const int rc = ensure_more(ctx, who, pick_stream(ctx, stream))) return rc;
    if (const int rc = map_call_begin(ctx, who, in.n, in.slots, in.first_slot, stream, false, f)) return rc;
    SplitCloud *hc = ctx->h_split_clouds + (size_t)f->g * ctx->n_slots;
    SplitCloud *dc = ctx->d_split_clouds + (size_t)f->g * ctx->n_slots;
    for (int i = 0; i < in.n; ++i) {
        SplitCloud &c = hc[i];
        c.slot = f->hm[i].slot;
        c.n_points = in.n_points[i];
        c.fresh = f->hm[i].fresh;
        c.fresh_z = f->hm[i].fresh_z;
        c.has_tf = in.transforms ? 1 : 0;
        c.io_index = i;
        c.ox = in.origins ? in.origins[(size_t)3 * i] : 0.f;
        c.oy = in.origins ? in.origins[(size_t)3 * i + 1] : 0.f;
        c.pos_x = ctx->pos_x[c.slot];
        c.pos_y = ctx->pos_y[c.slot];
        for (int k = 0; k < 12; ++k) c.tf[k] = in.transforms ? in.transforms[(size_t)12 * i + k] : 0.0;
    }
    HIPCHK(ctx, hipMemcpyAsync(dc, hc, sizeof(SplitCloud) * in.n, hipMemcpyHostToDevice, f->st));
    const int nch = std::max(1, (max_n + ctx->arena.PW - 1) / ctx->arena.PW); // (<= NCH: n_points <= max_points.  At least one: the split writes an empty cloud's counts)
    *cl = CloudArgs{dc, in.point_format, in.d_points, in.cloud_stride, in.d_labels, in.d_label_masks, nch};
    return GG_OK;
}

// The ground and the non-ground points of many labelled clouds as dense clouds (k12_split.hip), in the frame of the export: nothing is
// synchronised, no map is filled, no per-call layer is read (the lazily kept ones stay pending) and no host-side flag changes.
int gg_split_clouds(gg_context *ctx, const gg_cloud_split *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_split_clouds";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cloud_split");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    if (!x->d_counts) return fail(ctx, GG_ERR_INVALID, who, "d_counts is required");
    MapCall f;
    SplitArgs sa;
    const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms, x->d_labels, x->d_label_masks};
    if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &sa.cl)) return rc;
    sa.set[0] = SplitSet{x->ground.d_points, x->ground.d_height, x->ground.d_source};
    sa.set[1] = SplitSet{x->nonground.d_points, x->nonground.d_height, x->nonground.d_source};
    sa.counts = x->d_counts;
    sa.chunk_counts = ctx->d_split_counts + (size_t)f.g * ctx->n_slots * (size_t)std::max(ctx->arena.NCH, 1);
    launch_split(ctx->arena, sa, x->n, f.st);
    return map_call_end(ctx, f);
}

// The obstacle grid of many labelled clouds as dense planes (k13_raster.hip), in the same frame and with the same per-cloud records: nothing
// is synchronised, no map is filled or read beyond its `ground` layer, and no host-side flag (fresh, lazy_pending, liveness) changes.
int gg_rasterize_clouds(gg_context *ctx, const gg_cloud_raster *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_rasterize_clouds";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cloud_raster");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    if (!x->d_dst) return fail(ctx, GG_ERR_INVALID, who, "d_dst is null");
    if (x->channel_mask == 0u || (x->channel_mask >> GG_NUM_RASTER_CHANNELS) != 0u) return fail(ctx, GG_ERR_INVALID, who, "channel_mask");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->plane_stride < (size_t)ctx->arena.g.C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    MapCall f;
    RasterArgs ra;
    const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms, x->d_labels, x->d_label_masks};
    if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &ra.cl)) return rc;
    ra.channel_mask = x->channel_mask;
    ra.n_planes = 0;
    for (int ch = 0; ch < GG_NUM_RASTER_CHANNELS; ++ch) ra.plane_of[ch] = ((x->channel_mask >> ch) & 1u) ? ra.n_planes++ : -1;
    ra.order = x->order;
    ra.planes = reinterpret_cast<uint32_t *>(x->d_dst);
    ra.plane_stride = x->plane_stride;
    launch_raster(ctx->arena, ra, x->n, f.st);
    return map_call_end(ctx, f);
}

// gg_cluster_clouds' root counters, at its first call (alloc_call_scratch: nothing of the context changes when it fails)
static int ensure_cluster_scratch(gg_context *ctx, const char *who, hipStream_t st)
{
    if (ctx->cluster_mem.dev) return GG_OK;
    const int chunks = (ctx->arena.g.C + CLUSTER_CHUNK_CELLS - 1) / CLUSTER_CHUNK_CELLS;
    // (... and behind them one word per map and ring entry: the region count of gg_cluster_planes, which has no d_n_clusters to keep it in)
    const size_t words = (size_t)PARAM_RING * ctx->n_slots * ((size_t)chunks + 1);
    if (const int rc = alloc_call_scratch(ctx, who, st, words * sizeof(uint32_t), 64, {}, &ctx->cluster_mem, nullptr)) return rc;
    ctx->d_cluster_counts = (uint32_t *)ctx->cluster_mem.dev.get();
    ctx->d_region_counts = (int32_t *)(ctx->d_cluster_counts + (size_t)PARAM_RING * ctx->n_slots * (size_t)chunks);
    ctx->cluster_cell_chunks = chunks;
    return GG_OK;
}

// The obstacle clusters of many labelled clouds (k15_cluster.hip), in the frame of gg_rasterize_clouds and with the same per-cloud records:
// nothing is synchronised, no map is filled or read beyond its `ground` layer, and no host-side flag (fresh, lazy_pending, liveness) changes.
int gg_cluster_clouds(gg_context *ctx, const gg_cloud_clusters *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_cluster_clouds";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cloud_clusters");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    if (!x->d_cell_cluster || !x->d_n_clusters) return fail(ctx, GG_ERR_INVALID, who, "d_cell_cluster and d_n_clusters are required");
    if (x->min_points < 1) return fail(ctx, GG_ERR_INVALID, who, "min_points < 1");
    if (x->min_height != x->min_height || x->max_height != x->max_height) return fail(ctx, GG_ERR_INVALID, who, "min_height or max_height is NaN");
    if (x->connectivity != 4 && x->connectivity != 8) return fail(ctx, GG_ERR_INVALID, who, "connectivity is 4 or 8");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->plane_stride < (size_t)ctx->arena.g.C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->max_clusters < 0) return fail(ctx, GG_ERR_INVALID, who, "max_clusters < 0");
    if (x->d_clusters && x->max_clusters == 0) return fail(ctx, GG_ERR_INVALID, who, "d_clusters is given with max_clusters == 0");
    MapCall f;
    ClusterArgs ca;
    const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms, x->d_labels, x->d_label_masks};
    if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &ca.cl, ensure_cluster_scratch)) return rc;
    ca.min_points = x->min_points;
    ca.min_height = x->min_height;
    ca.max_height = x->max_height;
    ca.connectivity = x->connectivity;
    ca.order = x->order;
    ca.planes = reinterpret_cast<uint32_t *>(x->d_cell_cluster);
    ca.plane_stride = x->plane_stride;
    ca.point_cluster = x->d_point_cluster;
    ca.n_clusters = x->d_n_clusters;
    ca.records = reinterpret_cast<uint32_t *>(x->d_clusters);
    ca.max_clusters = x->d_clusters ? x->max_clusters : 0; // (without a table the kernels rank and count only)
    ca.cell_chunks = ctx->cluster_cell_chunks;
    ca.chunk_counts = ctx->d_cluster_counts + (size_t)f.g * ctx->n_slots * (size_t)ctx->cluster_cell_chunks;
    launch_cluster(ctx->arena, ca, x->n, f.st);
    return map_call_end(ctx, f);
}

// The connected regions of any plane of many maps (k26_regions.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none of
// which is read, as gg_fuse_states; the forest, its scratch and four of its launches are gg_cluster_clouds'.  Nothing is synchronised, no
// map is filled and no host-side flag changes.
int gg_cluster_planes(gg_context *ctx, const gg_plane_clusters *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_cluster_planes";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_plane_clusters");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    if (!x->d_seeds || !x->d_cell_cluster) return fail(ctx, GG_ERR_INVALID, who, "d_seeds and d_cell_cluster are required");
    if (x->lo > x->hi) return fail(ctx, GG_ERR_INVALID, who, "lo > hi");
    if (x->connectivity != 4 && x->connectivity != 8) return fail(ctx, GG_ERR_INVALID, who, "connectivity is 4 or 8");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->seed_stride < C) return fail(ctx, GG_ERR_INVALID, who, "seed_stride is smaller than rows * cols");
    if (x->plane_stride < C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->d_values && x->value_stride < C) return fail(ctx, GG_ERR_INVALID, who, "value_stride is smaller than rows * cols");
    if (x->d_cell_size && x->size_stride < C) return fail(ctx, GG_ERR_INVALID, who, "size_stride is smaller than rows * cols");
    if (x->min_cells < 1) return fail(ctx, GG_ERR_INVALID, who, "min_cells < 1");
    if (x->min_cells > 1 && !x->d_cell_size) return fail(ctx, GG_ERR_INVALID, who, "min_cells > 1 needs d_cell_size: it is the working memory of the filter");
    if (x->max_regions < 0) return fail(ctx, GG_ERR_INVALID, who, "max_regions < 0");
    if (x->d_regions && x->max_regions == 0) return fail(ctx, GG_ERR_INVALID, who, "d_regions is given with max_regions == 0");
    if (reinterpret_cast<uintptr_t>(x->d_regions) % 8 != 0) return fail(ctx, GG_ERR_INVALID, who, "d_regions is not 8-byte aligned");
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_seeds", x->d_seeds, n, x->seed_stride, C, false),
                                  plane_range("d_values", x->d_values, n, x->value_stride, C, false),
                                  plane_range("d_cell_cluster", x->d_cell_cluster, n, x->plane_stride, C, true),
                                  plane_range("d_cell_size", x->d_cell_size, n, x->size_stride, C, true),
                                  row_range("d_heads", x->d_heads, n, 4 * sizeof(int32_t), true),
                                  row_range("d_regions", x->d_regions, n, (size_t)x->max_regions * sizeof(gg_region), true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = ensure_cluster_scratch(ctx, who, pick_stream(ctx, stream))) return rc; // (checked arguments first, and no ring entry taken yet)
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    RegionArgs ra{};
    ra.forest.connectivity = x->connectivity;
    ra.forest.order = x->order;
    ra.forest.planes = reinterpret_cast<uint32_t *>(x->d_cell_cluster);
    ra.forest.plane_stride = x->plane_stride;
    ra.forest.n_clusters = ctx->d_region_counts + (size_t)f.g * ctx->n_slots;
    ra.forest.cell_chunks = ctx->cluster_cell_chunks;
    ra.forest.chunk_counts = ctx->d_cluster_counts + (size_t)f.g * ctx->n_slots * (size_t)ctx->cluster_cell_chunks;
    ra.seeds = x->d_seeds;
    ra.seed_stride = x->seed_stride;
    ra.lo = x->lo;
    ra.hi = x->hi;
    ra.min_cells = x->min_cells;
    ra.values = x->d_values;
    ra.value_stride = x->value_stride;
    ra.sizes = reinterpret_cast<uint32_t *>(x->d_cell_size);
    ra.size_stride = x->size_stride;
    ra.heads = x->d_heads;
    ra.records = reinterpret_cast<uint32_t *>(x->d_regions);
    ra.max_regions = x->d_regions ? x->max_regions : 0; // (without a table the kernels rank and count only)
    ra.tile = ctx->regions_tile;
    launch_regions(ctx->arena, ra, n, f.st);
    return map_call_end(ctx, f);
}

// The obstacle distance field of many maps (k16_clearance.hip).  Cloud mode: the frame of gg_cluster_clouds with the same per-cloud records
// and the same occupancy launches, on the d_dist2 planes.  Seed mode: a ring entry and the ordering of the export for maps 0 .. n-1, none of
// which is read.  Nothing is synchronised, no map is filled and no host-side flag changes in either.
int gg_clearance_clouds(gg_context *ctx, const gg_cloud_clearance *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_clearance_clouds";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cloud_clearance");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const bool from_clouds = x->d_points != nullptr;
    if (from_clouds == (x->d_seeds != nullptr)) return fail(ctx, GG_ERR_INVALID, who, "exactly one of d_points and d_seeds");
    if (!from_clouds && (x->n_points || x->transforms || x->d_labels || x->d_label_masks || x->slots))
        return fail(ctx, GG_ERR_INVALID, who, "a cloud member is set together with d_seeds");
    if (!from_clouds && x->seed_stride < C) return fail(ctx, GG_ERR_INVALID, who, "seed_stride is smaller than rows * cols");
    if (!x->d_dist2) return fail(ctx, GG_ERR_INVALID, who, "d_dist2 is required");
    if (x->plane_stride < C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->max_cells < 0) return fail(ctx, GG_ERR_INVALID, who, "max_cells < 0");
    if (from_clouds && x->min_points < 1) return fail(ctx, GG_ERR_INVALID, who, "min_points < 1");
    if (from_clouds && (x->min_height != x->min_height || x->max_height != x->max_height)) return fail(ctx, GG_ERR_INVALID, who, "min_height or max_height is NaN");
    MapCall f;
    ClearanceArgs ca{};
    ca.from_clouds = from_clouds;
    if (from_clouds) {
        const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms, x->d_labels, x->d_label_masks};
        if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &ca.occ.cl)) return rc;
        ca.occ.min_points = x->min_points;
        ca.occ.min_height = x->min_height;
        ca.occ.max_height = x->max_height;
        ca.occ.order = x->order;
        ca.occ.planes = reinterpret_cast<uint32_t *>(x->d_dist2);
        ca.occ.plane_stride = x->plane_stride;
        ca.occ.cell_chunks = (int)((C + CLUSTER_CHUNK_CELLS - 1) / CLUSTER_CHUNK_CELLS);
        ca.seeds = x->d_dist2; // (read in place)
        ca.seed_stride = x->plane_stride;
    } else {
        if (const int rc = map_call_begin(ctx, who, x->n, nullptr, 0, stream, false, &f)) return rc; // (GG_ERR_CAPACITY: n > n_slots)
        ca.seeds = x->d_seeds;
        ca.seed_stride = x->seed_stride;
    }
    const int cols = ctx->arena.g.cols;
    const bool bounded = x->max_cells > 0 && x->max_cells < cols; // (max_cells >= cols: no row holds a cell that far)
    ca.order = x->order;
    ca.reach = bounded ? x->max_cells : cols;
    ca.reach2 = (uint32_t)std::min<uint64_t>(x->max_cells > 0 ? (uint64_t)x->max_cells * (uint64_t)x->max_cells : ~0ull, (uint64_t)GG_CLEARANCE_NONE - 1);
    ca.dist2 = x->d_dist2;
    ca.nearest = x->d_nearest;
    ca.distance = x->d_distance;
    ca.plane_stride = x->plane_stride;
    ca.n_occupied = x->d_n_occupied;
    launch_clearance(ctx->arena, ca, x->n, f.st);
    return map_call_end(ctx, f);
}

// The free, unknown and occupied cells of many labelled clouds (k17_visibility.hip), in the frame of gg_cluster_clouds with the same per-cloud
// records (plus the sensor) and the same occupancy launches, on the d_state planes.  Nothing is synchronised, no map is filled and no
// host-side flag changes.
int gg_visibility_clouds(gg_context *ctx, const gg_cloud_visibility *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_visibility_clouds";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cloud_visibility");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    if (!x->origins || !x->d_state) return fail(ctx, GG_ERR_INVALID, who, "origins and d_state are required");
    if (x->plane_stride < C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->max_cells < 0) return fail(ctx, GG_ERR_INVALID, who, "max_cells < 0");
    if (x->min_points < 1) return fail(ctx, GG_ERR_INVALID, who, "min_points < 1");
    if (x->min_height != x->min_height || x->max_height != x->max_height) return fail(ctx, GG_ERR_INVALID, who, "min_height or max_height is NaN");
    // one bit per cell in a work-group's LDS, and 2 n n + n < 2^24 along a ray (k17_visibility.hip): both hold up to a side of 1143
    if (C > VISIBILITY_MAX_CELLS) return fail(ctx, GG_ERR_GEOMETRY, who, "the map has more cells than a work-group's local memory has bits");
    MapCall f;
    VisibilityArgs va{};
    const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms, x->d_labels, x->d_label_masks, x->origins};
    if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &va.occ.cl)) return rc;
    va.occ.min_points = x->min_points;
    va.occ.min_height = x->min_height;
    va.occ.max_height = x->max_height;
    va.occ.order = x->order;
    va.occ.planes = reinterpret_cast<uint32_t *>(x->d_state);
    va.occ.plane_stride = x->plane_stride;
    va.occ.cell_chunks = (int)((C + CLUSTER_CHUNK_CELLS - 1) / CLUSTER_CHUNK_CELLS);
    va.order = x->order;
    va.max_cells = x->max_cells;
    va.state = va.occ.planes;
    va.plane_stride = x->plane_stride;
    va.counts = x->d_counts;
    va.bitmap_words = (int)((C + 31) / 32);
    launch_visibility(ctx->arena, va, x->n, f.st);
    return map_call_end(ctx, f);
}

// The evidence planes of many maps carried from one scan to the next (k18_fuse.hip): a ring entry and the ordering of the export for maps
// 0 .. n-1, none of which is read, as the seed mode of gg_clearance_clouds; the per-map shifts travel in the ring entry.  Nothing is
// synchronised, no map is filled and no host-side flag changes.
int gg_fuse_states(gg_context *ctx, const gg_state_fusion *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_fuse_states";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_state_fusion");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    constexpr int LIMIT = (1 << 30) - 1; // of every increment and bound: P -+ decay and D +- hit / miss stay inside an int32
    if (!x->d_state || !x->d_evidence_out) return fail(ctx, GG_ERR_INVALID, who, "d_state and d_evidence_out are required");
    if (x->state_stride < C) return fail(ctx, GG_ERR_INVALID, who, "state_stride is smaller than rows * cols");
    if (x->plane_stride < C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->hit < 0 || x->hit > LIMIT || x->miss < 0 || x->miss > LIMIT || x->decay < 0 || x->decay > LIMIT)
        return fail(ctx, GG_ERR_INVALID, who, "hit, miss and decay lie in [0, 2^30 - 1]");
    if (x->e_min > 0 || x->e_min < -LIMIT || x->e_max < 0 || x->e_max > LIMIT) return fail(ctx, GG_ERR_INVALID, who, "-(2^30 - 1) <= e_min <= 0 <= e_max <= 2^30 - 1");
    if (x->free_threshold > -1 || x->free_threshold < x->e_min) return fail(ctx, GG_ERR_INVALID, who, "e_min <= free_threshold <= -1");
    if (x->occ_threshold < 1 || x->occ_threshold > x->e_max) return fail(ctx, GG_ERR_INVALID, who, "1 <= occ_threshold <= e_max");
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    // the scroll reads d_evidence_in at shifted cells and the frontier reads neighbours, so no update in place is defined
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_state", x->d_state, n, x->state_stride, C, false),
                                  plane_range("d_evidence_in", x->d_evidence_in, n, x->plane_stride, C, false),
                                  plane_range("d_evidence_out", x->d_evidence_out, n, x->plane_stride, C, true),
                                  plane_range("d_fused", x->d_fused, n, x->plane_stride, C, true),
                                  plane_range("d_frontier", x->d_frontier, n, x->plane_stride, C, true),
                                  row_range("d_counts", x->d_counts, n, 4 * sizeof(int32_t), true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    FuseArgs fa{};
    if (x->shifts) { // (rows, cols) -> (along a line, across lines), clamped: from |s| = side on no prior lies inside the map
        int2 *hs = ring_entry(ctx->ring_shifts, f);
        for (int i = 0; i < n; ++i) {
            const Shift s = clamped_shift(x->shifts, i, rows, cols);
            hs[i] = row_major ? make_int2(s.s1, s.s0) : make_int2(s.s0, s.s1);
        }
        if (!(fa.shifts = ring_upload(ctx, ctx->ring_shifts, f, n))) return GG_ERR_HIP;
    }
    fa.state = x->d_state;
    fa.state_stride = x->state_stride;
    fa.evidence_in = x->d_evidence_in;
    fa.hit = x->hit;
    fa.miss = x->miss;
    fa.decay = x->decay;
    fa.e_min = x->e_min;
    fa.e_max = x->e_max;
    fa.free_threshold = x->free_threshold;
    fa.occ_threshold = x->occ_threshold;
    std::tie(fa.nx, fa.ny) = plane_sides(row_major, rows, cols);
    fa.tiles_x = (fa.nx + FUSE_TILE_X - 1) / FUSE_TILE_X;
    fa.evidence_out = x->d_evidence_out;
    fa.fused = x->d_fused;
    fa.frontier = x->d_frontier;
    fa.plane_stride = x->plane_stride;
    fa.counts = x->d_counts;
    launch_fuse(fa, n, f.st);
    return map_call_end(ctx, f);
}

// This scan's clusters associated with the last scan's (k23_tracks.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none
// of which is read, as gg_fuse_states; the per-map shifts travel in the ring entry.  Nothing is synchronised, no map is filled and no
// host-side flag changes.
int gg_track_clusters(gg_context *ctx, const gg_cluster_tracks *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_track_clusters";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cluster_tracks");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_cells || !x->d_tracks_out || !x->d_heads_out) return fail(ctx, GG_ERR_INVALID, who, "d_cells, d_tracks_out and d_heads_out are required");
    const bool prior = x->d_cells_prev != nullptr;
    if (prior != (x->d_tracks_in != nullptr) || prior != (x->d_heads_in != nullptr))
        return fail(ctx, GG_ERR_INVALID, who, "d_cells_prev, d_tracks_in and d_heads_in are given together or not at all");
    if (x->cells_stride < C) return fail(ctx, GG_ERR_INVALID, who, "cells_stride is smaller than rows * cols");
    if (prior && x->prev_stride < C) return fail(ctx, GG_ERR_INVALID, who, "prev_stride is smaller than rows * cols");
    if (x->d_cell_track && x->track_stride < C) return fail(ctx, GG_ERR_INVALID, who, "track_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->max_clusters < 1 || x->max_clusters > GG_TRACK_MAX_CLUSTERS) return fail(ctx, GG_ERR_INVALID, who, "max_clusters lies in [1, 1024]");
    if (x->gate < 0 || x->gate > 4) return fail(ctx, GG_ERR_INVALID, who, "gate lies in [0, 4]");
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    // the coordinate sums of a cluster (and its overlap, <= 81 cells) must stay inside an int32
    if ((uint64_t)C * (uint64_t)std::max(rows, cols) > 0x7FFFFFFFull) return fail(ctx, GG_ERR_GEOMETRY, who, "rows * cols * max(rows, cols) exceeds 2^31 - 1");
    const int n = x->n;
    const size_t M = (size_t)x->max_clusters;
    const BufferRange ranges[] = {plane_range("d_cells", x->d_cells, n, x->cells_stride, C, false),
                                  plane_range("d_cells_prev", x->d_cells_prev, n, x->prev_stride, C, false),
                                  row_range("d_tracks_in", x->d_tracks_in, n, M * sizeof(gg_track), false),
                                  row_range("d_heads_in", x->d_heads_in, n, 4 * sizeof(int32_t), false),
                                  row_range("d_tracks_out", x->d_tracks_out, n, M * sizeof(gg_track), true),
                                  row_range("d_heads_out", x->d_heads_out, n, 4 * sizeof(int32_t), true),
                                  plane_range("d_cell_track", x->d_cell_track, n, x->track_stride, C, true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    TrackArgs ta{};
    if (x->shifts) { // (rows, cols) -> (along a line, across lines), clamped: from |s| = side on nothing overlaps
        int2 *hs = ring_entry(ctx->ring_shifts, f);
        for (int i = 0; i < n; ++i) {
            const Shift s = clamped_shift(x->shifts, i, rows, cols);
            hs[i] = row_major ? make_int2(s.s1, s.s0) : make_int2(s.s0, s.s1);
        }
        if (!(ta.shifts = ring_upload(ctx, ctx->ring_shifts, f, n))) return GG_ERR_HIP;
    }
    ta.cells = x->d_cells;
    ta.cells_stride = x->cells_stride;
    ta.prev = x->d_cells_prev;
    ta.prev_stride = x->prev_stride;
    ta.tracks_in = x->d_tracks_in;
    ta.heads_in = x->d_heads_in;
    std::tie(ta.nx, ta.ny) = plane_sides(row_major, rows, cols);
    ta.row_major = row_major ? 1 : 0;
    ta.M = x->max_clusters;
    ta.gate = x->gate;
    ta.slab_words = (int)std::min<size_t>(M * M, (size_t)TRACK_SLAB_WORDS);
    ta.tracks_out = x->d_tracks_out;
    ta.heads_out = x->d_heads_out;
    ta.cell_track = x->d_cell_track;
    ta.track_stride = x->track_stride;
    launch_tracks(ta, n, f.st);
    return map_call_end(ctx, f);
}

// The oriented boxes of the obstacle clusters of many clouds (k24_boxes.hip), in the frame of gg_split_clouds with the same per-cloud records
// and without labels (the ids stand in where the frame wants a label pointer): nothing is synchronised, no map is filled, no layer is read and no host-side flag changes.
int gg_box_clusters(gg_context *ctx, const gg_cluster_boxes *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_box_clusters";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_cluster_boxes");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    if (!x->d_point_cluster || !x->d_n_clusters || !x->d_boxes) return fail(ctx, GG_ERR_INVALID, who, "d_point_cluster, d_n_clusters and d_boxes are required");
    if (!x->rotations) return fail(ctx, GG_ERR_INVALID, who, "rotations is required");
    if (x->n_rotations < 1 || x->n_rotations > GG_BOX_MAX_HEADINGS) return fail(ctx, GG_ERR_INVALID, who, "n_rotations lies in [1, 32]");
    for (int k = 0; k < 2 * x->n_rotations; ++k)
        if (x->rotations[k] < -GG_MATCH_UNIT || x->rotations[k] > GG_MATCH_UNIT) return fail(ctx, GG_ERR_INVALID, who, "a rotation word lies outside [-16384, 16384]");
    if (x->criterion != GG_BOX_AREA && x->criterion != GG_BOX_EDGE) return fail(ctx, GG_ERR_INVALID, who, "criterion");
    if (x->max_clusters < 1 || x->max_clusters > GG_BOX_MAX_CLUSTERS) return fail(ctx, GG_ERR_INVALID, who, "max_clusters lies in [1, 4096]");
    // |u| <= 8 * side + 1, so both projections stay inside an int32 (k24_boxes.hip relies on it)
    if (ctx->arena.g.rows > BOX_MAX_SIDE || ctx->arena.g.cols > BOX_MAX_SIDE) return fail(ctx, GG_ERR_GEOMETRY, who, "the map has more than 4096 rows or columns");
    const int n = x->n, K = x->n_rotations;
    const size_t M = (size_t)x->max_clusters;
    if (x->cloud_stride > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, who, "cloud_stride is larger than max_points"); // (the frame's, ahead of the ranges it sizes)
    if (x->d_points && x->n <= ctx->n_slots) { // (a null d_points and n > n_slots are refused by the frame below)
        const size_t rec = x->point_format == GG_POINT16 ? sizeof(gg_point16) : sizeof(gg_point32);
        const BufferRange ranges[] = {row_range("d_points", x->d_points, n, x->cloud_stride * rec, false),
                                      row_range("d_point_cluster", x->d_point_cluster, n, x->cloud_stride * sizeof(int32_t), false),
                                      row_range("d_n_clusters", x->d_n_clusters, n, sizeof(int32_t), false),
                                      row_range("d_boxes", x->d_boxes, n, M * sizeof(gg_box), true),
                                      row_range("d_costs", x->d_costs, n, M * K * sizeof(uint64_t), true)};
        if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    }
    MapCall f;
    BoxArgs ba;
    // The frame is entered as it stands.  It asks for exactly one of labels and masks and reads neither; this call has no labels, so the ids
    // stand in for the label bytes: CloudArgs::labels is then not null and k24_boxes.hip never looks at it.
    const LabelledClouds in{x->n, x->first_slot, x->slots, x->point_format, x->d_points, x->cloud_stride, x->n_points, x->transforms,
                            reinterpret_cast<const uint8_t *>(x->d_point_cluster), nullptr};
    if (const int rc = labelled_clouds_begin(ctx, who, in, stream, &f, &ba.cl)) return rc;
    ba.point_cluster = x->d_point_cluster;
    ba.n_clusters = x->d_n_clusters;
    ba.K = K;
    ba.criterion = x->criterion;
    ba.M = x->max_clusters;
    ba.slab = box_slab_clusters(K, x->max_clusters);
    ba.scale = (double)GG_BOX_UNIT / ctx->arena.g.resolution;
    for (int k = 0; k < 2 * GG_BOX_MAX_HEADINGS; ++k) ba.rot[k] = k < 2 * K ? x->rotations[k] : 0;
    ba.boxes = x->d_boxes;
    ba.costs = reinterpret_cast<unsigned long long *>(x->d_costs);
    launch_boxes(ctx->arena, ba, n, f.st);
    return map_call_end(ctx, f);
}

// The cost-to-go fields and paths of many maps (k19_route.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none of which
// is read, as gg_fuse_states; the per-map start cells travel in the ring entry.  Nothing is synchronised, no map is filled and no host-side
// flag changes.
int gg_route_planes(gg_context *ctx, const gg_plane_routes *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_route_planes";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_plane_routes");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_goals || !x->d_dist) return fail(ctx, GG_ERR_INVALID, who, "d_goals and d_dist are required");
    if (x->d_blocked && x->blocked_stride < C) return fail(ctx, GG_ERR_INVALID, who, "blocked_stride is smaller than rows * cols");
    if (x->d_cost && x->cost_stride < C) return fail(ctx, GG_ERR_INVALID, who, "cost_stride is smaller than rows * cols");
    if (x->goal_stride < C) return fail(ctx, GG_ERR_INVALID, who, "goal_stride is smaller than rows * cols");
    if (x->plane_stride < C) return fail(ctx, GG_ERR_INVALID, who, "plane_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->connectivity != 4 && x->connectivity != 8) return fail(ctx, GG_ERR_INVALID, who, "connectivity is 4 or 8");
    const bool diagonals = x->connectivity == 8;
    if (x->straight < 1 || x->straight > 65535 || (diagonals && (x->diagonal < 1 || x->diagonal > 65535)))
        return fail(ctx, GG_ERR_INVALID, who, "straight and diagonal lie in [1, 65535]");
    if (x->cost_max < 1) return fail(ctx, GG_ERR_INVALID, who, "cost_max < 1");
    if (x->max_cost < 0) return fail(ctx, GG_ERR_INVALID, who, "max_cost < 0");
    // every true D fits an int32 and the unsigned sum of a stored word and one step cannot wrap (k19_route.hip relies on it).  The product of
    // the first two factors is < 2^47, so the test by division is exact and nothing here overflows
    const uint64_t step_max = (uint64_t)std::max(x->straight, diagonals ? x->diagonal : 0) * (uint64_t)x->cost_max;
    if (step_max > (uint64_t)GG_ROUTE_NONE - 1 || step_max > ((uint64_t)GG_ROUTE_NONE - 1) / (uint64_t)C)
        return fail(ctx, GG_ERR_INVALID, who, "max(straight, diagonal) * cost_max * rows * cols exceeds 2^31 - 2");
    if (x->starts) {
        if (!x->d_paths || !x->d_path_len || x->max_path < 1) return fail(ctx, GG_ERR_INVALID, who, "starts needs d_paths, d_path_len and max_path >= 1");
        if (x->n <= ctx->n_slots) // (beyond that the call is refused below, and starts[] is the caller's to size by n)
            for (int i = 0; i < x->n; ++i)
                if (x->starts[i] < -1 || (int64_t)x->starts[i] >= (int64_t)C) return fail(ctx, GG_ERR_INVALID, who, "a start lies outside [-1, rows * cols)");
    }
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    RouteArgs ra{};
    std::tie(ra.nx, ra.ny) = plane_sides(row_major, rows, cols);
    ra.tiles_x = (ra.nx + ROUTE_TILE - 1) / ROUTE_TILE;
    ra.tiles_y = (ra.ny + ROUTE_TILE - 1) / ROUTE_TILE;
    if ((int64_t)ra.tiles_x * ra.tiles_y > ROUTE_MAX_TILES) return fail(ctx, GG_ERR_GEOMETRY, who, "the map has more than 4096 tiles of 64 x 64 cells");
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_blocked", x->d_blocked, n, x->blocked_stride, C, false),
                                  plane_range("d_cost", x->d_cost, n, x->cost_stride, C, false),
                                  plane_range("d_goals", x->d_goals, n, x->goal_stride, C, false),
                                  plane_range("d_dist", x->d_dist, n, x->plane_stride, C, true),
                                  plane_range("d_next", x->d_next, n, x->plane_stride, C, true),
                                  row_range("d_counts", x->d_counts, n, 3 * sizeof(int32_t), true),
                                  row_range("d_paths", x->starts ? x->d_paths : nullptr, n, (size_t)x->max_path * sizeof(int32_t), true),
                                  row_range("d_path_len", x->starts ? x->d_path_len : nullptr, n, sizeof(int32_t), true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    if (x->starts) {
        std::copy(x->starts, x->starts + n, ring_entry(ctx->ring_starts, f));
        if (!(ra.starts = ring_upload(ctx, ctx->ring_starts, f, n))) return GG_ERR_HIP;
        ra.paths = x->d_paths;
        ra.max_path = x->max_path;
        ra.path_len = x->d_path_len;
    }
    ra.blocked = x->d_blocked;
    ra.blocked_stride = x->blocked_stride;
    ra.cost = x->d_cost;
    ra.cost_stride = x->cost_stride;
    ra.goals = x->d_goals;
    ra.goal_stride = x->goal_stride;
    ra.row_major = row_major;
    ra.diagonals = diagonals;
    ra.straight = (uint32_t)x->straight;
    ra.diagonal = diagonals ? (uint32_t)x->diagonal : 0u;
    ra.cost_max = x->cost_max;
    ra.reach = x->max_cost > 0 ? (uint32_t)x->max_cost : (uint32_t)GG_ROUTE_NONE - 1u;
    ra.dist = x->d_dist;
    ra.next = x->d_next;
    ra.plane_stride = x->plane_stride;
    ra.counts = x->d_counts;
    launch_route(ra, n, f.st);
    return map_call_end(ctx, f);
}

// The best alignment of many scans to their grids (k20_match.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none of
// which is read, as gg_route_planes; the per-map shifts and pivots and the rotation table travel in the ring entry, and so do the partial
// results between the two launches.  Nothing is synchronised, no map is filled and no host-side flag changes.
int gg_match_planes(gg_context *ctx, const gg_plane_matches *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_match_planes";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_plane_matches");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_scan || !x->d_field || !x->d_best) return fail(ctx, GG_ERR_INVALID, who, "d_scan, d_field and d_best are required");
    if (x->scan_stride < C) return fail(ctx, GG_ERR_INVALID, who, "scan_stride is smaller than rows * cols");
    if (x->field_stride < C) return fail(ctx, GG_ERR_INVALID, who, "field_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->window < 0 || x->window > MATCH_MAX_WINDOW) return fail(ctx, GG_ERR_INVALID, who, "window lies in [0, 32]");
    if (x->rotations ? (x->n_rotations < 1 || x->n_rotations > MATCH_MAX_ROTATIONS) : x->n_rotations != 0)
        return fail(ctx, GG_ERR_INVALID, who, "n_rotations lies in [1, 64] with rotations and is 0 without");
    for (int k = 0; k < 2 * x->n_rotations; ++k)
        if (x->rotations[k] < -GG_MATCH_UNIT || x->rotations[k] > GG_MATCH_UNIT) return fail(ctx, GG_ERR_INVALID, who, "a rotation word lies outside [-16384, 16384]");
    // every score fits an int32: at most rows * cols scan cells of at most field_max each (the test by division is exact)
    if (x->field_max < 1 || (uint64_t)x->field_max > (uint64_t)INT32_MAX / (uint64_t)C) return fail(ctx, GG_ERR_INVALID, who, "field_max < 1 or field_max * rows * cols exceeds 2^31 - 1");
    // cq dr - sq dc and sq dr + cq dc stay inside an int32 (k20_match.hip relies on it)
    if (rows > 32768 || cols > 32768) return fail(ctx, GG_ERR_GEOMETRY, who, "the map has more than 32768 rows or columns");
    const int K = x->rotations ? x->n_rotations : 1, D = 2 * x->window + 1;
    const size_t volume = (size_t)K * D * D;
    if (x->d_scores && x->score_stride < volume) return fail(ctx, GG_ERR_INVALID, who, "score_stride is smaller than n_rotations * (2 * window + 1)^2");
    if (x->pivots && x->n <= ctx->n_slots) // (beyond that the call is refused below, and pivots[] is the caller's to size by n)
        for (int i = 0; i < x->n; ++i) {
            const int32_t pr = x->pivots[2 * (size_t)i], pc = x->pivots[2 * (size_t)i + 1];
            if (pr < 0 || pr >= rows || pc < 0 || pc >= cols) return fail(ctx, GG_ERR_INVALID, who, "a pivot lies outside the map");
        }
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_scan", x->d_scan, n, x->scan_stride, C, false), plane_range("d_field", x->d_field, n, x->field_stride, C, false),
                                  plane_range("d_best", x->d_best, n, 6, 6, true), plane_range("d_scores", x->d_scores, n, x->score_stride, volume, true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    MatchArgs ma{};
    if (x->shifts) { // clamped as gg_fuse_states clamps them, and kept in (rows, cols) whatever the order: the kernel works in (row, col)
        int2 *hs = ring_entry(ctx->ring_shifts, f);
        for (int i = 0; i < n; ++i) {
            const Shift s = clamped_shift(x->shifts, i, rows, cols);
            hs[i] = make_int2(s.s0, s.s1);
        }
        if (!(ma.shifts = ring_upload(ctx, ctx->ring_shifts, f, n))) return GG_ERR_HIP;
    }
    if (x->pivots) {
        int2 *hp = ring_entry(ctx->ring_pivots, f);
        for (int i = 0; i < n; ++i) hp[i] = make_int2(x->pivots[2 * (size_t)i], x->pivots[2 * (size_t)i + 1]);
        if (!(ma.pivots = ring_upload(ctx, ctx->ring_pivots, f, n))) return GG_ERR_HIP;
    }
    if (x->rotations) {
        int2 *hr = ring_entry(ctx->ring_rotations, f);
        for (int k = 0; k < K; ++k) hr[k] = make_int2(x->rotations[2 * (size_t)k], x->rotations[2 * (size_t)k + 1]);
        if (!(ma.rotations = ring_upload(ctx, ctx->ring_rotations, f, K))) return GG_ERR_HIP;
    }
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    ma.scan = x->d_scan;
    ma.scan_stride = x->scan_stride;
    ma.field = x->d_field;
    ma.field_stride = x->field_stride;
    ma.field_max = x->field_max;
    ma.n_rotations = K;
    ma.window = x->window;
    std::tie(ma.nx, ma.ny) = plane_sides(row_major, rows, cols);
    ma.row_major = row_major;
    ma.partials = ctx->d_match_partials + (size_t)f.g * ctx->n_slots * MATCH_MAX_ROTATIONS;
    ma.best = x->d_best;
    ma.scores = x->d_scores;
    ma.score_stride = x->score_stride;
    launch_match(ma, n, f.st);
    return map_call_end(ctx, f);
}

// The span table of a rectangle for gg_footprint_planes: host integer arithmetic only, no context
int gg_footprint_spans(const int32_t *rotations, int n_rotations, const int32_t rect[4], int radius, int32_t *spans, int *needed)
{
    constexpr int BOX = FOOTPRINT_MAX_RADIUS + 1; // the test is evaluated on [-33, 33]^2
    if (!rotations || !rect) return GG_ERR_INVALID;
    if (n_rotations < 1 || n_rotations > FOOTPRINT_MAX_HEADINGS) return GG_ERR_INVALID;
    for (int k = 0; k < 2 * n_rotations; ++k)
        if (rotations[k] < -GG_MATCH_UNIT || rotations[k] > GG_MATCH_UNIT) return GG_ERR_INVALID;
    for (int k = 0; k < 4; ++k)
        if (rect[k] < -(1 << 30) || rect[k] > (1 << 30)) return GG_ERR_INVALID;
    if (rect[0] > rect[1] || rect[2] > rect[3]) return GG_ERR_INVALID;
    if (spans && (radius < 0 || radius > FOOTPRINT_MAX_RADIUS)) return GG_ERR_INVALID;
    std::vector<int32_t> lo((size_t)n_rotations * (2 * BOX + 1)), hi(lo.size()); // (min b, max b) of row a of heading k; (1, 0): empty
    int need = -1;
    for (int k = 0; k < n_rotations; ++k) {
        const int32_t cq = rotations[2 * k], sq = rotations[2 * k + 1];
        for (int a = -BOX; a <= BOX; ++a) {
            int32_t first = 1, last = 0;
            for (int b = -BOX; b <= BOX; ++b) {
                const int32_t u = cq * a + sq * b, v = -sq * a + cq * b;
                if (u < rect[0] || u > rect[1] || v < rect[2] || v > rect[3]) continue;
                if (first > last) first = b;
                last = b;
                need = std::max(need, std::max(std::abs(a), std::abs(b)));
            }
            lo[(size_t)k * (2 * BOX + 1) + a + BOX] = first;
            hi[(size_t)k * (2 * BOX + 1) + a + BOX] = last;
        }
    }
    if (needed) *needed = need;
    if (!spans) return GG_OK;
    if (need > radius) return GG_ERR_INVALID;
    const int D = 2 * radius + 1;
    for (int k = 0; k < n_rotations; ++k)
        for (int a = -radius; a <= radius; ++a) {
            spans[((size_t)k * D + a + radius) * 2] = lo[(size_t)k * (2 * BOX + 1) + a + BOX];
            spans[((size_t)k * D + a + radius) * 2 + 1] = hi[(size_t)k * (2 * BOX + 1) + a + BOX];
        }
    return GG_OK;
}

// Which headings a footprint fits, per cell (k21_footprint.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none of which
// is read, as gg_route_planes and gg_match_planes; the span table travels in the ring entry, per line offset of the plane (transposed for
// column-major planes: column-convexity makes that exact) and packed (footprint_pack).  Nothing is synchronised, no map is filled and no
// host-side flag changes.
int gg_footprint_planes(gg_context *ctx, const gg_plane_footprints *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_footprint_planes";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_plane_footprints");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_blocked) return fail(ctx, GG_ERR_INVALID, who, "d_blocked is required");
    if (!x->spans) return fail(ctx, GG_ERR_INVALID, who, "spans is required");
    if (!x->d_mask && !x->d_fit && !x->d_counts) return fail(ctx, GG_ERR_INVALID, who, "at least one of d_mask, d_fit and d_counts must be given");
    if (x->blocked_stride < C) return fail(ctx, GG_ERR_INVALID, who, "blocked_stride is smaller than rows * cols");
    if (x->d_mask && x->mask_stride < C) return fail(ctx, GG_ERR_INVALID, who, "mask_stride is smaller than rows * cols");
    if (x->d_fit && x->fit_stride < C) return fail(ctx, GG_ERR_INVALID, who, "fit_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->n_headings < 1 || x->n_headings > FOOTPRINT_MAX_HEADINGS) return fail(ctx, GG_ERR_INVALID, who, "n_headings lies in [1, 32]");
    if (x->radius < 0 || x->radius > FOOTPRINT_MAX_RADIUS) return fail(ctx, GG_ERR_INVALID, who, "radius lies in [0, 32]");
    if (x->min_fit < 1 || x->min_fit > x->n_headings) return fail(ctx, GG_ERR_INVALID, who, "min_fit lies in [1, n_headings]");
    if (x->outside_free != 0 && x->outside_free != 1) return fail(ctx, GG_ERR_INVALID, who, "outside_free is 0 or 1");
    const int K = x->n_headings, R = x->radius, D = 2 * R + 1;
    // the rows as given, the columns they make (the transposed table), and column-convexity: the rows that hold column b are consecutive
    std::vector<int32_t> across((size_t)K * D * 2);
    for (int k = 0; k < K; ++k) {
        const int32_t *sp = x->spans + (size_t)k * D * 2;
        int32_t *tr = across.data() + (size_t)k * D * 2;
        for (int b = 0; b < D; ++b) tr[2 * b] = 1, tr[2 * b + 1] = 0;
        for (int a = -R; a <= R; ++a) {
            const int32_t lo = sp[2 * (a + R)], hi = sp[2 * (a + R) + 1];
            if (lo > hi) continue;
            if (lo < -R || hi > R) return fail(ctx, GG_ERR_INVALID, who, "a span reaches beyond the radius");
            for (int b = lo; b <= hi; ++b) {
                int32_t *t = tr + 2 * (b + R);
                if (t[0] > t[1]) t[0] = t[1] = a;
                else if (t[1] == a - 1) t[1] = a;
                else return fail(ctx, GG_ERR_INVALID, who, "a heading of the span table is not column-convex");
            }
        }
    }
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    // (one input and outputs only: every pair of the table holds an output, so every pair is tested)
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_blocked", x->d_blocked, n, x->blocked_stride, C, false), plane_range("d_mask", x->d_mask, n, x->mask_stride, C, true),
                                  plane_range("d_fit", x->d_fit, n, x->fit_stride, C, true), plane_range("d_counts", x->d_counts, n, 3, 3, true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    uint32_t *ht = ring_entry(ctx->ring_footprint, f);
    const int32_t *per_line = row_major ? x->spans : across.data();
    int n_levels = 1;
    for (int e = 0; e < K * D; ++e) {
        ht[e] = footprint_pack(per_line[2 * e], per_line[2 * e + 1]);
        if (ht[e] != FOOTPRINT_EMPTY) n_levels = std::max(n_levels, (int)(ht[e] >> 16) + 1);
    }
    FootprintArgs fa{};
    if (!(fa.table = ring_upload(ctx, ctx->ring_footprint, f, K * D))) return GG_ERR_HIP;
    fa.blocked = x->d_blocked;
    fa.blocked_stride = x->blocked_stride;
    fa.n_headings = K;
    fa.radius = R;
    fa.n_levels = n_levels;
    fa.min_fit = x->min_fit;
    fa.outside_free = x->outside_free;
    std::tie(fa.nx, fa.ny) = plane_sides(row_major, rows, cols);
    fa.tiles_x = (fa.nx + FOOTPRINT_TILE - 1) / FOOTPRINT_TILE;
    fa.mask = x->d_mask;
    fa.mask_stride = x->mask_stride;
    fa.fit = x->d_fit;
    fa.fit_stride = x->fit_stride;
    fa.counts = x->d_counts;
    launch_footprint(fa, n, f.st);
    return map_call_end(ctx, f);
}

// The move table of a car-like vehicle for gg_route_headings: host integer arithmetic only, no context
int gg_heading_moves(const int32_t *rotations, int n_rotations, int step, int unit, int turn, int reverse_pct, int spin, int32_t *moves)
{
    if (!rotations || !moves) return GG_ERR_INVALID;
    if (n_rotations < 1 || n_rotations > HEADINGS_MAX) return GG_ERR_INVALID;
    for (int k = 0; k < 2 * n_rotations; ++k)
        if (rotations[k] < -GG_MATCH_UNIT || rotations[k] > GG_MATCH_UNIT) return GG_ERR_INVALID;
    if (step < 1 || step > HEADINGS_MAX_STEP || unit < 1 || unit > 1024 || turn < 0 || spin < 0) return GG_ERR_INVALID;
    if (reverse_pct != 0 && reverse_pct < 100) return GG_ERR_INVALID;
    const int K = n_rotations;
    const auto rha = [](int32_t v) { return v < 0 ? -((-v + GG_MATCH_UNIT / 2) >> 14) : (v + GG_MATCH_UNIT / 2) >> 14; };
    std::vector<int32_t> table((size_t)K * HEADINGS_MAX_MOVES * 4, 0);
    bool fits = true;
    const auto put = [&](int k, int m, int da, int db, int k2, int64_t s) {
        int32_t *e = table.data() + ((size_t)k * HEADINGS_MAX_MOVES + m) * 4;
        if (s > HEADINGS_MAX_COST) fits = false;
        e[0] = da, e[1] = db, e[2] = k2, e[3] = (int32_t)std::min<int64_t>(s, HEADINGS_MAX_COST);
    };
    for (int k = 0; k < K; ++k) {
        const int da = rha(step * rotations[2 * k]), db = rha(step * rotations[2 * k + 1]);
        const int left = (k + 1) % K, right = (k + K - 1) % K;
        if (da != 0 || db != 0) {
            const int64_t sq = (int64_t)unit * unit * (da * da + db * db); // <= 2^20 * 18
            int64_t root = (int64_t)std::sqrt((double)sq);
            while (root * root > sq) --root;
            while ((root + 1) * (root + 1) <= sq) ++root;
            const int64_t s = std::max<int64_t>(1, root), st = s + turn;
            put(k, 0, da, db, k, s);
            put(k, 1, da, db, left, st);
            put(k, 2, da, db, right, st);
            if (reverse_pct) {
                const auto back = [&](int64_t c) { return (c * reverse_pct + 99) / 100; };
                put(k, 3, -da, -db, k, back(s));
                put(k, 4, -da, -db, left, back(st));
                put(k, 5, -da, -db, right, back(st));
            }
        }
        if (spin && K > 1) {
            put(k, 6, 0, 0, left, spin);
            put(k, 7, 0, 0, right, spin);
        }
    }
    if (!fits) return GG_ERR_INVALID;
    std::copy(table.begin(), table.end(), moves);
    return GG_OK;
}

// The cost-to-go over cells and headings of many maps (k22_headings.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none
// of which is read, as gg_route_planes and gg_footprint_planes; the move table travels in the ring entry in (line, position) offsets (da and
// db swapped for column-major planes) and packed (headings_pack), and so do the start poses.  Nothing is synchronised, no map is filled and
// no host-side flag changes.
int gg_route_headings(gg_context *ctx, const gg_heading_routes *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_route_headings";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_heading_routes");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_mask || !x->d_goals || !x->d_dist) return fail(ctx, GG_ERR_INVALID, who, "d_mask, d_goals and d_dist are required");
    if (!x->moves) return fail(ctx, GG_ERR_INVALID, who, "moves is required");
    if (x->n_headings < 1 || x->n_headings > HEADINGS_MAX) return fail(ctx, GG_ERR_INVALID, who, "n_headings lies in [1, 32]");
    const int K = x->n_headings;
    if (x->mask_stride < C) return fail(ctx, GG_ERR_INVALID, who, "mask_stride is smaller than rows * cols");
    if (x->d_cost && x->cost_stride < C) return fail(ctx, GG_ERR_INVALID, who, "cost_stride is smaller than rows * cols");
    if (x->goal_stride < C) return fail(ctx, GG_ERR_INVALID, who, "goal_stride is smaller than rows * cols");
    if (x->plane_stride < C || x->dist_stride / (size_t)K < x->plane_stride) return fail(ctx, GG_ERR_INVALID, who, "plane_stride >= rows * cols and dist_stride >= n_headings * plane_stride");
    if (x->d_next && (x->next_plane_stride < C || x->next_stride / (size_t)K < x->next_plane_stride))
        return fail(ctx, GG_ERR_INVALID, who, "next_plane_stride >= rows * cols and next_stride >= n_headings * next_plane_stride");
    if (x->d_best && x->best_stride < C) return fail(ctx, GG_ERR_INVALID, who, "best_stride is smaller than rows * cols");
    if (x->d_best_heading && x->best_heading_stride < C) return fail(ctx, GG_ERR_INVALID, who, "best_heading_stride is smaller than rows * cols");
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->cost_max < 1) return fail(ctx, GG_ERR_INVALID, who, "cost_max < 1");
    if (x->max_cost < 0) return fail(ctx, GG_ERR_INVALID, who, "max_cost < 0");
    int s_max = 0;
    for (int k = 0; k < K; ++k)
        for (int m = 0; m < HEADINGS_MAX_MOVES; ++m) {
            const int32_t *e = x->moves + ((size_t)k * HEADINGS_MAX_MOVES + m) * 4;
            if (e[3] == 0) continue; // an absent entry: its other words are not looked at
            if (e[3] < 1 || e[3] > HEADINGS_MAX_COST) return fail(ctx, GG_ERR_INVALID, who, "a move's cost lies outside [1, 32767]");
            if (std::abs(e[0]) > HEADINGS_MAX_STEP || std::abs(e[1]) > HEADINGS_MAX_STEP) return fail(ctx, GG_ERR_INVALID, who, "a move is longer than 3 cells");
            if (e[2] < 0 || e[2] >= K) return fail(ctx, GG_ERR_INVALID, who, "a move's heading lies outside [0, n_headings)");
            if (e[0] == 0 && e[1] == 0 && e[2] == k) return fail(ctx, GG_ERR_INVALID, who, "a move leads to its own state");
            s_max = std::max(s_max, e[3]);
        }
    // every true D fits an int32 and the unsigned sum of a stored word and one move cannot wrap (k22_headings.hip relies on it).  The product
    // of the first two factors is < 2^46, so the test by division is exact and nothing here overflows
    const uint64_t step_max = (uint64_t)s_max * (uint64_t)x->cost_max, states = (uint64_t)C * (uint64_t)K;
    if (step_max > (uint64_t)GG_ROUTE_NONE - 1 || step_max > ((uint64_t)GG_ROUTE_NONE - 1) / states)
        return fail(ctx, GG_ERR_INVALID, who, "max s * cost_max * rows * cols * n_headings exceeds 2^31 - 2");
    if (x->starts) {
        if (!x->d_paths || !x->d_path_len || x->max_len < 1) return fail(ctx, GG_ERR_INVALID, who, "starts needs d_paths, d_path_len and max_len >= 1");
        if (x->path_stride / 2 < (size_t)x->max_len) return fail(ctx, GG_ERR_INVALID, who, "path_stride is smaller than 2 * max_len");
        if (x->n <= ctx->n_slots) // (beyond that the call is refused below, and starts[] is the caller's to size by n)
            for (int i = 0; i < x->n; ++i) {
                const int32_t cell = x->starts[2 * i], heading = x->starts[2 * i + 1];
                if (cell < -1 || (int64_t)cell >= (int64_t)C) return fail(ctx, GG_ERR_INVALID, who, "a start cell lies outside [-1, rows * cols)");
                if (cell >= 0 && (heading < 0 || heading >= K)) return fail(ctx, GG_ERR_INVALID, who, "a start heading lies outside [0, n_headings)");
            }
    }
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    const bool row_major = x->order == GG_PLANES_ROWMAJOR;
    HeadingsArgs ha{};
    std::tie(ha.nx, ha.ny) = plane_sides(row_major, rows, cols);
    ha.tile = headings_tile(K);
    ha.tiles_x = (ha.nx + ha.tile - 1) / ha.tile;
    ha.tiles_y = (ha.ny + ha.tile - 1) / ha.tile;
    if ((int64_t)ha.tiles_x * ha.tiles_y > HEADINGS_MAX_TILES) return fail(ctx, GG_ERR_GEOMETRY, who, "the map has more than 4096 tiles");
    // (d_dist and d_next: K planes per map, so a map's last plane ends (K - 1) plane strides and a plane into it)
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_mask", x->d_mask, n, x->mask_stride, C, false),
                                  plane_range("d_cost", x->d_cost, n, x->cost_stride, C, false),
                                  plane_range("d_goals", x->d_goals, n, x->goal_stride, C, false),
                                  plane_range("d_dist", x->d_dist, n, x->dist_stride, (size_t)(K - 1) * x->plane_stride + C, true),
                                  plane_range("d_next", x->d_next, n, x->next_stride, (size_t)(K - 1) * x->next_plane_stride + C, true),
                                  plane_range("d_best", x->d_best, n, x->best_stride, C, true),
                                  plane_range("d_best_heading", x->d_best_heading, n, x->best_heading_stride, C, true),
                                  row_range("d_counts", x->d_counts, n, 3 * sizeof(int32_t), true),
                                  plane_range("d_paths", x->starts ? x->d_paths : nullptr, n, x->path_stride, 2 * (size_t)x->max_len, true),
                                  row_range("d_path_len", x->starts ? x->d_path_len : nullptr, n, sizeof(int32_t), true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    uint32_t *ht = ring_entry(ctx->ring_moves, f);
    for (int k = 0; k < K; ++k) {
        // the heading's first translating move decides how a slot walks the tile for it: along the axis the move is longer in, against the move
        int first_line = 0, first_pos = 0;
        uint8_t walk = 0;
        for (int m = 0; m < HEADINGS_MAX_MOVES; ++m) {
            const int32_t *e = x->moves + ((size_t)k * HEADINGS_MAX_MOVES + m) * 4;
            const int d_line = row_major ? e[0] : e[1], d_pos = row_major ? e[1] : e[0];
            ht[k * HEADINGS_MAX_MOVES + m] = e[3] == 0 ? 0u : headings_pack(d_line, d_pos, e[2], e[3]);
            if (e[3] == 0 || (d_line == 0 && d_pos == 0)) continue;
            const bool positions = std::abs(d_pos) > std::abs(d_line);
            if (first_line == 0 && first_pos == 0) {
                first_line = d_line, first_pos = d_pos;
                walk = (positions ? HEADINGS_WALK_POSITIONS : 0) | ((positions ? d_pos : d_line) > 0 ? HEADINGS_WALK_BACK : 0);
                continue;
            }
            const bool first_positions = (walk & HEADINGS_WALK_POSITIONS) != 0;
            if (positions != first_positions) walk |= HEADINGS_WALK_ALT_AXIS;
            if ((first_positions ? d_pos * first_pos : d_line * first_line) < 0) walk |= HEADINGS_WALK_ALT_DIR;
        }
        ha.walk[k] = walk;
    }
    if (!(ha.table = ring_upload(ctx, ctx->ring_moves, f, K * HEADINGS_MAX_MOVES))) return GG_ERR_HIP;
    if (x->starts) {
        int2 *hs = ring_entry(ctx->ring_poses, f);
        for (int i = 0; i < n; ++i) hs[i] = make_int2(x->starts[2 * i], x->starts[2 * i] >= 0 ? x->starts[2 * i + 1] : 0);
        if (!(ha.starts = ring_upload(ctx, ctx->ring_poses, f, n))) return GG_ERR_HIP;
        ha.paths = x->d_paths;
        ha.path_stride = x->path_stride;
        ha.max_len = x->max_len;
        ha.path_len = x->d_path_len;
    }
    ha.mask = x->d_mask;
    ha.mask_stride = x->mask_stride;
    ha.cost = x->d_cost;
    ha.cost_stride = x->cost_stride;
    ha.goals = x->d_goals;
    ha.goal_stride = x->goal_stride;
    ha.goal_headings = x->goal_headings;
    ha.n_headings = K;
    ha.cost_max = x->cost_max;
    ha.reach = x->max_cost > 0 ? (uint32_t)x->max_cost : (uint32_t)GG_ROUTE_NONE - 1u;
    ha.max_rounds = (int)std::min<uint64_t>(states, (uint64_t)GG_ROUTE_NONE - 1);
    ha.max_sweeps = K * ha.tile * ha.tile;
    ha.dist = x->d_dist;
    ha.dist_stride = x->dist_stride;
    ha.plane_stride = x->plane_stride;
    ha.next = x->d_next;
    ha.next_stride = x->next_stride;
    ha.next_plane_stride = x->next_plane_stride;
    ha.best = x->d_best;
    ha.best_stride = x->best_stride;
    ha.best_heading = x->d_best_heading;
    ha.best_heading_stride = x->best_heading_stride;
    ha.counts = x->d_counts;
    launch_headings(ha, n, f.st);
    return map_call_end(ctx, f);
}

// The score of candidate trajectories of many maps (k25_rollouts.hip): a ring entry and the ordering of the export for maps 0 .. n-1, none
// of which is read, as gg_route_headings; the starts and, in the relative frame, the rotation table travel in the ring entry.  The
// rollout table is the caller's device data and is not looked at here.  Nothing is synchronised, no map is filled and no host-side flag
// changes.
int gg_score_rollouts(gg_context *ctx, const gg_rollouts *x, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    const char *who = "gg_score_rollouts";
    if (!x) return fail(ctx, GG_ERR_INVALID, who, "null gg_rollouts");
    if (x->n < 0) return fail(ctx, GG_ERR_INVALID, who, "n < 0");
    if (x->n == 0) return GG_OK;
    const size_t C = (size_t)ctx->arena.g.C;
    const int rows = ctx->arena.g.rows, cols = ctx->arena.g.cols;
    if (!x->d_mask || !x->d_table || !x->d_records || !x->starts) return fail(ctx, GG_ERR_INVALID, who, "d_mask, d_table, d_records and starts are required");
    if (x->frame != GG_ROLLOUTS_RELATIVE && x->frame != GG_ROLLOUTS_ABSOLUTE) return fail(ctx, GG_ERR_INVALID, who, "frame");
    const bool relative = x->frame == GG_ROLLOUTS_RELATIVE;
    if (relative && !x->rotations) return fail(ctx, GG_ERR_INVALID, who, "rotations is required in the relative frame");
    if (x->n_headings < 1 || x->n_headings > HEADINGS_MAX) return fail(ctx, GG_ERR_INVALID, who, "n_headings lies in [1, 32]");
    if (x->n_rollouts < 1 || x->n_rollouts > GG_ROLLOUTS_MAX) return fail(ctx, GG_ERR_INVALID, who, "n_rollouts lies in [1, 65536]");
    if (x->n_steps < 1 || x->n_steps > GG_ROLLOUTS_MAX_STEPS) return fail(ctx, GG_ERR_INVALID, who, "n_steps lies in [1, 128]");
    const int K = x->n_headings, P = x->n_rollouts, T = x->n_steps;
    if (x->order != GG_PLANES_COLMAJOR && x->order != GG_PLANES_ROWMAJOR) return fail(ctx, GG_ERR_INVALID, who, "order");
    if (x->reach < 0 || x->reach > GG_ROLLOUTS_MAX_REACH) return fail(ctx, GG_ERR_INVALID, who, "reach lies in [0, 63]");
    if (x->mask_stride < C) return fail(ctx, GG_ERR_INVALID, who, "mask_stride is smaller than rows * cols");
    if (x->d_cost && x->cost_stride < C) return fail(ctx, GG_ERR_INVALID, who, "cost_stride is smaller than rows * cols");
    if (x->d_dist && (x->plane_stride < C || x->dist_stride / (size_t)K < x->plane_stride))
        return fail(ctx, GG_ERR_INVALID, who, "plane_stride >= rows * cols and dist_stride >= n_headings * plane_stride");
    if (x->d_clear && x->clear_stride < C) return fail(ctx, GG_ERR_INVALID, who, "clear_stride is smaller than rows * cols");
    const size_t table_words = 4 * (size_t)P * (size_t)T; // <= 2^25
    if (x->table_stride != 0 && x->table_stride < table_words) return fail(ctx, GG_ERR_INVALID, who, "table_stride is 0 or >= 4 * n_rollouts * n_steps");
    if (x->record_stride < 8 * (size_t)P) return fail(ctx, GG_ERR_INVALID, who, "record_stride is smaller than 8 * n_rollouts");
    if (relative)
        for (int k = 0; k < 2 * K; ++k)
            if (x->rotations[k] < -GG_MATCH_UNIT || x->rotations[k] > GG_MATCH_UNIT) return fail(ctx, GG_ERR_INVALID, who, "a rotation word lies outside [-16384, 16384]");
    // the sum of a rollout's step costs fits an int32 (k25_rollouts.hip relies on it)
    if (x->cost_max < 1 || (uint64_t)T * 32767u * (uint64_t)x->cost_max > (uint64_t)GG_ROUTE_NONE - 1)
        return fail(ctx, GG_ERR_INVALID, who, "cost_max < 1 or n_steps * 32767 * cost_max exceeds 2^31 - 2");
    if (x->n <= ctx->n_slots) // (beyond that the call is refused below, and starts[] is the caller's to size by n)
        for (int i = 0; i < x->n; ++i) {
            const int32_t *s = x->starts + 3 * (size_t)i;
            if (s[0] == -1) continue;
            if (s[0] < 0 || (int64_t)s[0] >= 16 * (int64_t)rows || s[1] < 0 || (int64_t)s[1] >= 16 * (int64_t)cols) return fail(ctx, GG_ERR_INVALID, who, "a start lies outside the map");
            if (s[2] < 0 || s[2] >= K) return fail(ctx, GG_ERR_INVALID, who, "a start heading lies outside [0, n_headings)");
        }
    if (x->n > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, who, "n is larger than n_slots");
    const int n = x->n;
    const BufferRange ranges[] = {plane_range("d_mask", x->d_mask, n, x->mask_stride, C, false),
                                  plane_range("d_cost", x->d_cost, n, x->cost_stride, C, false),
                                  plane_range("d_dist", x->d_dist, n, x->dist_stride, (size_t)(K - 1) * x->plane_stride + C, false),
                                  plane_range("d_clear", x->d_clear, n, x->clear_stride, C, false),
                                  plane_range("d_table", x->d_table, n, x->table_stride, table_words, false),
                                  plane_range("d_records", x->d_records, n, x->record_stride, 8 * (size_t)P, true),
                                  row_range("d_best", x->d_best, n, 4 * sizeof(int32_t), true)};
    if (const int rc = check_no_overlap(ctx, who, ranges)) return rc;
    MapCall f;
    if (const int rc = map_call_begin(ctx, who, n, nullptr, 0, stream, false, &f)) return rc;
    RolloutArgs ra{};
    int32_t *hs = ring_entry(ctx->ring_rollout_starts, f);
    for (int i = 0; i < n; ++i) {
        const int32_t *s = x->starts + 3 * (size_t)i;
        const bool given = s[0] != -1;
        hs[3 * i] = s[0], hs[3 * i + 1] = given ? s[1] : 0, hs[3 * i + 2] = given ? s[2] : 0;
    }
    if (!(ra.starts = ring_upload(ctx, ctx->ring_rollout_starts, f, 3 * n))) return GG_ERR_HIP;
    if (relative) {
        int2 *hr = ring_entry(ctx->ring_rotations, f);
        for (int k = 0; k < K; ++k) hr[k] = make_int2(x->rotations[2 * (size_t)k], x->rotations[2 * (size_t)k + 1]);
        if (!(ra.rotations = ring_upload(ctx, ctx->ring_rotations, f, K))) return GG_ERR_HIP;
    }
    ra.mask = x->d_mask;
    ra.mask_stride = x->mask_stride;
    ra.cost = x->d_cost;
    ra.cost_stride = x->cost_stride;
    ra.dist = x->d_dist;
    ra.dist_stride = x->dist_stride;
    ra.plane_stride = x->plane_stride;
    ra.clear = x->d_clear;
    ra.clear_stride = x->clear_stride;
    ra.table = x->d_table;
    ra.table_stride = x->table_stride;
    ra.rows = rows, ra.cols = cols;
    ra.row_major = x->order == GG_PLANES_ROWMAJOR;
    ra.K = K, ra.P = P, ra.T = T;
    ra.frame = x->frame;
    ra.reach = x->reach;
    ra.cost_max = x->cost_max;
    ra.records = x->d_records;
    ra.record_stride = x->record_stride;
    ra.best = x->d_best;
    launch_rollouts(ra, n, f.st);
    return map_call_end(ctx, f);
}

int gg_get_map_position(const gg_context *ctx, int slot, double *pos_x, double *pos_y)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (pos_x) *pos_x = ctx->pos_x[slot];
    if (pos_y) *pos_y = ctx->pos_y[slot];
    return GG_OK;
}

int gg_set_layer(gg_context *ctx, int slot, int layer, const float *src)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!src || layer < 0 || layer >= GG_NUM_LAYERS) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    if (layer == GG_LAYER_GROUNDPATCH) ctx->no_confidence[slot] = 0, ctx->gp_tainted[slot] = 1;
    // both kinds of layer have a device representation of their own (sheared pairs / sparse tile blocks): converted at the host boundary
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_image, src, (size_t)ctx->arena.g.C * 4, hipMemcpyHostToDevice, ctx->stream));
    if (const int rc = insert_planes(ctx, slot, 1u << layer, ctx->d_image, (size_t)ctx->arena.g.C, ctx->stream)) return rc;
    HIPCHK(ctx, hipGetLastError());
    if (const int rc = own_stream_mutated_map(ctx)) return rc;
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

int gg_get_layer(gg_context *ctx, int slot, int layer, float *dst)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!dst || layer < 0 || layer >= GG_NUM_LAYERS) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    // both kinds of layer have a device representation of their own (sheared pairs / sparse tile blocks): extract the dense plane
    if (const int rc = extract_planes(ctx, slot, 1u << layer, ctx->d_image, (size_t)ctx->arena.g.C, ctx->stream)) return rc;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(dst, ctx->d_image, (size_t)ctx->arena.g.C * 4, hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// d_planes / h_planes at their first use: GG_NUM_LAYERS dense planes, `plane_floats` apart, on the device and in pinned host memory
static size_t plane_floats(const gg_context *ctx) { return align_up((size_t)ctx->arena.g.C * 4, 256) / 4; }
static int ensure_plane_staging(gg_context *ctx)
{
    const size_t bytes = (size_t)GG_NUM_LAYERS * plane_floats(ctx) * sizeof(float);
    if (!ctx->d_planes) HIPCHK(ctx, ctx->d_planes.create(bytes));
    if (!ctx->h_planes) HIPCHK(ctx, ctx->h_planes.create(bytes));
    return GG_OK;
}
// Planes that came down into h_planes move on to the caller's, on the context's host threads: plane src[k] of the staging block to dst[k]
// (which need not be aligned: it may sit inside a serialised message), for k < n_want
static void copy_staged_planes(gg_context *ctx, void *const dst[], const int src[], int n_want, size_t plane)
{
    const size_t C = (size_t)ctx->arena.g.C;
    if (n_want == 0) return;
    ctx->helper.split((size_t)n_want * C, [&](size_t lo, size_t hi) {
        for (size_t k = lo / C; k < (size_t)n_want && k * C < hi; ++k) {
            const size_t a0 = std::max(lo, k * C) - k * C, a1 = std::min(hi, (k + 1) * C) - k * C;
            memcpy((char *)dst[k] + a0 * sizeof(float), ctx->h_planes + (size_t)src[k] * plane + a0, (a1 - a0) * sizeof(float));
        }
    });
}

// dst[l] (nullable) receives layer l
static int get_layers_impl(gg_context *ctx, int slot, void *const dst[GG_NUM_LAYERS])
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    const size_t plane = plane_floats(ctx);
    if (const int rc = ensure_plane_staging(ctx)) return rc;
    // The requested planes are extracted side by side, come down in ONE copy into pinned memory (a copy into the caller's
    // pageable matrices is staged by the runtime in small pieces: 0.7 ms for eleven 364 x 364 layers, against 0.15 ms), and the
    // context's host threads move them on to where the caller wants them.
    void *to[GG_NUM_LAYERS];
    int from[GG_NUM_LAYERS], n_want = 0;
    unsigned want_mask = 0u;
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!dst[l]) continue;
        want_mask |= 1u << l;
        to[n_want] = dst[l];
        from[n_want] = n_want; // (plane k = the k-th requested layer)
        ++n_want;
    }
    if (n_want == 0) return GG_OK;
    if (const int rc = extract_planes(ctx, slot, want_mask, ctx->d_planes, plane, ctx->stream)) return rc; // (plane k = the k-th requested layer)
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_planes, ctx->d_planes, (size_t)n_want * plane * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    copy_staged_planes(ctx, to, from, n_want, plane);
    return GG_OK;
}

int gg_get_layers(gg_context *ctx, int slot, float *const dst[GG_NUM_LAYERS])
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!dst) return GG_ERR_INVALID;
    void *d[GG_NUM_LAYERS];
    for (int l = 0; l < GG_NUM_LAYERS; ++l) d[l] = dst[l];
    return get_layers_impl(ctx, slot, d);
}

// grid_map_msgs/GridMap, ROS 1 serialisation (include/groundgrid_hip.h): the skeleton is written by the host, the layer planes land
// in their data[] arrays straight from the pinned download
int gg_get_gridmap_message(gg_context *ctx, int slot, unsigned layer_mask, const gg_gridmap_header *header, uint8_t *dst, size_t capacity, size_t *size)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!size) return fail(ctx, GG_ERR_INVALID, "gg_get_gridmap_message: null size");
    static const char *const names[GG_NUM_LAYERS] = {"points", "ground", "groundpatch", "minGroundHeight", "maxGroundHeight", "groundCandidates",
                                                     "planeDist", "m2", "meanVariance", "pointsRaw", "variance"}; // src/GroundGrid.cpp:55, src/GroundSegmentation.cpp:61-75
    if (layer_mask == 0u) layer_mask = (1u << GG_NUM_LAYERS) - 1u;
    layer_mask &= (1u << GG_NUM_LAYERS) - 1u;
    const gg_gridmap_header none{};
    const gg_gridmap_header &h = header ? *header : none;
    const char *frame = h.frame_id ? h.frame_id : "map";
    const Geometry &g = ctx->arena.g;
    const size_t C = (size_t)g.C;
    // two passes over the same writer: the first only measures
    size_t data_at[GG_NUM_LAYERS] = {};
    auto write = [&](uint8_t *out) -> size_t {
        size_t at = 0;
        auto put = [&](const void *p, size_t n) {
            if (out) memcpy(out + at, p, n);
            at += n;
        };
        auto u32 = [&](uint32_t v) { put(&v, 4); };
        auto f64 = [&](double v) { put(&v, 8); };
        auto str = [&](const char *t) {
            u32((uint32_t)strlen(t));
            put(t, strlen(t));
        };
        u32(h.seq); // info.header
        u32(h.stamp_sec);
        u32(h.stamp_nsec);
        str(frame);
        f64(g.resolution);
        f64(g.length0);
        f64(g.length1);
        f64(ctx->pos_x[slot]); // pose.position
        f64(ctx->pos_y[slot]);
        f64(0.0);
        f64(0.0); // pose.orientation
        f64(0.0);
        f64(0.0);
        f64(1.0);
        u32((uint32_t)__builtin_popcount(layer_mask)); // layers
        for (int l = 0; l < GG_NUM_LAYERS; ++l)
            if ((layer_mask >> l) & 1u) str(names[l]);
        u32((uint32_t)__builtin_popcount(h.basic_layers & layer_mask)); // basic_layers
        for (int l = 0; l < GG_NUM_LAYERS; ++l)
            if ((h.basic_layers & layer_mask) >> l & 1u) str(names[l]);
        u32((uint32_t)__builtin_popcount(layer_mask)); // data
        for (int l = 0; l < GG_NUM_LAYERS; ++l) {
            if (!((layer_mask >> l) & 1u)) continue;
            u32(2u); // layout.dim (GridMapMsgHelpers: column-major storage -> "column_index" first)
            str("column_index");
            u32((uint32_t)g.cols);
            u32((uint32_t)C);
            str("row_index");
            u32((uint32_t)g.rows);
            u32((uint32_t)g.rows);
            u32(0u); // layout.data_offset
            u32((uint32_t)C);
            data_at[l] = at;
            at += C * 4;
        }
        const uint16_t zero = 0;
        put(&zero, 2); // outer_start_index
        put(&zero, 2); // inner_start_index
        return at;
    };
    const size_t need = write(nullptr);
    *size = need;
    if (!dst) return GG_OK;
    if (capacity < need) return fail(ctx, GG_ERR_CAPACITY, "gg_get_gridmap_message: buffer smaller than the message");
    write(dst);
    void *planes[GG_NUM_LAYERS];
    for (int l = 0; l < GG_NUM_LAYERS; ++l) planes[l] = ((layer_mask >> l) & 1u) ? (void *)(dst + data_at[l]) : nullptr;
    return get_layers_impl(ctx, slot, planes);
}

int gg_get_layer_image_u8(gg_context *ctx, int slot, int layer, uint8_t *dst, float *lower, float *upper)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!dst || layer < 0 || layer >= GG_NUM_LAYERS) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    const Geometry &g = ctx->arena.g;
    uint8_t *d_img = reinterpret_cast<uint8_t *>(ctx->d_image);
    if (const int rc = extract_planes(ctx, slot, 1u << layer, ctx->d_scroll_scratch, (size_t)g.C, ctx->stream)) return rc;
    launch_layer_to_u8(ctx->d_scroll_scratch, g.rows, g.cols, ctx->d_bounds, d_img, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    float b[2];
    HIPCHK(ctx, hipMemcpyAsync(dst, d_img, (size_t)g.C, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b, ctx->d_bounds, sizeof b, hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (lower) *lower = b[0];
    if (upper) *upper = b[1];
    return GG_OK;
}

int gg_get_terrain_image(gg_context *ctx, int slot, float *dst)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!dst) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    const Geometry &g = ctx->arena.g;
    launch_terrain_image(ctx->arena, slot, ctx->d_image, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(dst, ctx->d_image, (size_t)g.C * 3 * 4, hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// The gg_batch of the single-cloud host entry points: one cloud of n32 packed points at d_points for `slot`.  The caller adds its outputs
static gg_batch single_cloud_batch(const gg_context *ctx, int slot, const gg_point16 *d_points, const int32_t *n32, const float origin[3], const double *base_z,
                                   const double *tf)
{
    gg_batch b{};
    b.n_clouds = 1;
    b.first_slot = slot;
    b.point_format = GG_POINT16;
    b.d_points = d_points;
    b.cloud_stride = ctx->max_points;
    b.n_points = n32;
    b.origins = origin;
    b.base_z = base_z;
    b.transforms = tf;
    return b;
}

// records [lo, hi) of a sensor_msgs/PointCloud2 payload -> the packed records the device reads
static void unpack_pc2(const uint8_t *data, size_t lo, size_t hi, size_t point_step, size_t off_x, size_t off_y, size_t off_z, size_t off_ring, gg_point16 *dst)
{
    for (size_t i = lo; i < hi; ++i) {
        const uint8_t *p = data + i * point_step;
        gg_point16 &d = dst[i];
        memcpy(&d.x, p + off_x, 4);
        memcpy(&d.y, p + off_y, 4);
        memcpy(&d.z, p + off_z, 4);
        memcpy(&d.ring, p + off_ring, 2);
        d.pad = 0;
    }
}

// sensor_msgs/PointCloud2 payload -> the packed records the device reads, in one host pass (the reference goes
// wire -> 32-byte PCL points first, pcl::fromROSMsg at src/GroundGridNodelet.cpp:120)
int gg_filter_cloud_pc2(gg_context *ctx, int slot, const uint8_t *data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                        size_t off_z, size_t off_ring, const double *map_from_cloud, const float origin[3], double base_z,
                        uint8_t *out_label, int32_t *out_index, size_t *out_n)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if ((!data && n) || !origin) return fail(ctx, GG_ERR_INVALID, "null data / origin");
    if (n > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, "cloud larger than max_points");
    if (off_x + 4 > point_step || off_y + 4 > point_step || off_z + 4 > point_step || off_ring + 2 > point_step)
        return fail(ctx, GG_ERR_INVALID, "field offset outside point_step");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unpack_pc2(data, 0, n, point_step, off_x, off_y, off_z, off_ring, ctx->h_stage_pts); // (serially, one upload: gg_filter_cloud_pc2_out differs)
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage_pts, ctx->h_stage_pts, n * sizeof(gg_point16), hipMemcpyHostToDevice, s));
    const int32_t n32 = (int32_t)n;
    gg_batch b = single_cloud_batch(ctx, slot, ctx->d_stage_pts, &n32, origin, &base_z, map_from_cloud);
    b.d_labels = ctx->d_stage_labels;
    b.d_out_index = ctx->d_stage_index;
    b.d_out_counts = ctx->d_stage_counts;
    const int rc = enqueue_batch(ctx, &b, s);
    if (rc != GG_OK) return rc;
    if (n && out_label) HIPCHK(ctx, hipMemcpyAsync(out_label, ctx->d_stage_labels, n, hipMemcpyDeviceToHost, s));
    if (n && out_index) HIPCHK(ctx, hipMemcpyAsync(out_index, ctx->d_stage_index, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_stage_counts, ctx->d_stage_counts, 16, hipMemcpyDeviceToHost, s));
    SYNCCHK(ctx, hipStreamSynchronize(s));
    if (out_n) *out_n = (size_t)ctx->h_stage_counts[0];
    return GG_OK;
}

// ... and with the returned cloud coming back as 18-byte PointCloud2 records written by the label kernel (gg_batch.d_out_pc2)
int gg_filter_cloud_pc2_out(gg_context *ctx, int slot, const uint8_t *data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                            size_t off_z, size_t off_ring, const double *map_from_cloud, const float origin[3], double base_z,
                            uint8_t *out_data, size_t *out_n)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if ((!data && n) || !origin || (!out_data && n)) return fail(ctx, GG_ERR_INVALID, "null data / origin / out_data");
    if (n > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, "cloud larger than max_points");
    if (off_x + 4 > point_step || off_y + 4 > point_step || off_z + 4 > point_step || off_ring + 2 > point_step)
        return fail(ctx, GG_ERR_INVALID, "field offset outside point_step");
    if (ctx->next_ticket != ctx->oldest_ticket) return fail(ctx, GG_ERR_INVALID, "gg_filter_cloud_pc2_out while async tickets are outstanding");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t block = 64 + ctx->max_points * GG_PC2_POINT_STEP;
    if (!ctx->d_pc2) HIPCHK(ctx, ctx->d_pc2.create(block));
    if (!ctx->h_pc2) HIPCHK(ctx, ctx->h_pc2.create(block));
    hipStream_t s = ctx->stream;
    for (int c = 0; c < 2; ++c) { // pack and upload in two pieces, as the 32-byte entry point does
        const size_t lo = n * c / 2, hi = n * (c + 1) / 2;
        if (hi == lo) continue;
        ctx->helper.split(hi - lo, [&](size_t a0, size_t a1) { unpack_pc2(data, lo + a0, lo + a1, point_step, off_x, off_y, off_z, off_ring, ctx->h_stage_pts); });
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage_pts + lo, ctx->h_stage_pts + lo, (hi - lo) * sizeof(gg_point16), hipMemcpyHostToDevice, s));
    }
    const int32_t n32 = (int32_t)n;
    gg_batch b = single_cloud_batch(ctx, slot, ctx->d_stage_pts, &n32, origin, &base_z, map_from_cloud);
    b.d_out_counts = reinterpret_cast<int32_t *>(ctx->d_pc2.get());
    b.d_out_pc2 = ctx->d_pc2 + 64;
    const int rc = enqueue_batch(ctx, &b, s);
    if (rc != GG_OK) return rc;
    // counts and records in one copy: the size of the returned cloud is only known on the device, and it is nearly n
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pc2, ctx->d_pc2, 64 + n * GG_PC2_POINT_STEP, hipMemcpyDeviceToHost, s));
    SYNCCHK(ctx, hipStreamSynchronize(s));
    const size_t got = (size_t)reinterpret_cast<const int32_t *>(ctx->h_pc2.get())[0];
    if (out_n) *out_n = got;
    const uint8_t *src = ctx->h_pc2 + 64;
    ctx->helper.split(got * GG_PC2_POINT_STEP, [&](size_t a0, size_t a1) { memcpy(out_data + a0, src + a0, a1 - a0); });
    return GG_OK;
}

int gg_get_expected_points(const gg_context *ctx, float *dst)
{
    if (!ctx || !dst) return GG_ERR_INVALID;
    memcpy(dst, ctx->h_expected.data(), ctx->h_expected.size() * 4);
    return GG_OK;
}

int gg_filter_batch(gg_context *ctx, const gg_batch *b, void *stream)
{
    if (!ctx || !b) return GG_ERR_INVALID;
    if (b->n_clouds < 0 || b->n_clouds > ctx->n_slots) return fail(ctx, GG_ERR_CAPACITY, "slot range");
    if (!b->slots && (b->first_slot < 0 || b->first_slot + b->n_clouds > ctx->n_slots)) return fail(ctx, GG_ERR_CAPACITY, "slot range");
    if (b->n_clouds == 0) return GG_OK;
    // (distinct and in range: two clouds of one launch on one map would race)
    if (const int rc = check_slot_list(ctx, "gg_filter_batch", b->n_clouds, b->slots, b->first_slot)) return rc;
    if (!b->d_points || !b->n_points || !b->origins || !b->base_z) return fail(ctx, GG_ERR_INVALID, "null batch field");
    if (b->point_format != GG_POINT32 && b->point_format != GG_POINT16) return fail(ctx, GG_ERR_INVALID, "point_format");
    if (b->d_out_clouds && b->point_format != GG_POINT32) return fail(ctx, GG_ERR_INVALID, "d_out_clouds needs GG_POINT32 input");
    if (b->d_label_masks && (b->cloud_stride & 3u)) return fail(ctx, GG_ERR_INVALID, "d_label_masks needs cloud_stride % 4 == 0");
    for (int i = 0; i < b->n_clouds; ++i)
        if (b->n_points[i] < 0 || (size_t)b->n_points[i] > ctx->max_points || (size_t)b->n_points[i] > b->cloud_stride)
            return fail(ctx, GG_ERR_CAPACITY, "n_points exceeds max_points / cloud_stride");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return enqueue_batch(ctx, b, pick_stream(ctx, stream), nullptr, true);
}

int gg_device_error(gg_context *ctx, int clear)
{
    if (!ctx || !ctx->h_dev_error) return GG_ERR_INVALID;
    const uint32_t code = *ctx->h_dev_error;
    if (clear) *ctx->h_dev_error = GG_DEVERR_NONE;
    return (int)code;
}

int gg_batch_fence(gg_context *ctx, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stream_waits_for_second_half(ctx, pick_stream(ctx, stream));
}

int gg_synchronize(gg_context *ctx)
{
    if (!ctx) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc; // batches on caller streams (and their second halves) included
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// one ticket: pack + upload, the seven kernels, the download.  `pipelined`: uploads and downloads on their own streams so that
// they overlap the neighbouring tickets' kernels (gg_filter_cloud_async); a synchronous call has nothing to overlap with and puts
// everything on the context's stream instead -- no cross-stream events (four API calls, ~15 us per cloud)
static int enqueue_ticket(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *tf, const float origin[3], double base_z,
                          int *ticket, bool pipelined, const LayerPlan *plan = nullptr)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if ((!cloud && n) || !origin || !ticket) return fail(ctx, GG_ERR_INVALID, "null cloud / origin / ticket");
    if (n > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, "cloud larger than max_points");
    if (ctx->next_ticket - ctx->oldest_ticket >= GG_ASYNC_DEPTH) return fail(ctx, GG_ERR_CAPACITY, "GG_ASYNC_DEPTH tickets outstanding: wait for the oldest first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (a synchronous call has no ticket outstanding: always the same staging set, so that its launches are one kind for the graph cache)
    const int set = pipelined ? ctx->next_ticket % GG_ASYNC_DEPTH : 0;
    ctx->slot_of_ticket[ctx->next_ticket % GG_ASYNC_DEPTH] = set;
    gg_context::AsyncSlot &as = ctx->async_slot[set];
    const ContextBuffers::AsyncSet &dev = ctx->async_set[set]; // (its device side)

    static const bool host_timing = getenv("GG_HOST_TIMING") != nullptr; // (tools: where does the host call spend its time)
    const auto t_pack0 = std::chrono::steady_clock::now();
    // pack and upload in pieces (each packed by all of the context's host threads): the copy of the first travels while the
    // second is packed (and all of it overlaps the device work of the previous ticket)
    const int pieces = std::max(1, std::min(ctx->upload_pieces, 8));
    for (int c = 0; c < pieces; ++c) {
        const size_t lo = n * c / pieces, hi = n * (c + 1) / pieces;
        if (hi == lo) continue;
        ctx->helper.split(hi - lo, [&](size_t a0, size_t a1) { pack_points(cloud + lo + a0, as.h_pts + lo + a0, a1 - a0); });
        HIPCHK(ctx, hipMemcpyAsync(dev.d_pts + lo, as.h_pts + lo, (hi - lo) * sizeof(gg_point16), hipMemcpyHostToDevice, pipelined ? ctx->h2d_stream : ctx->stream));
    }
    if (host_timing) ctx->host_t[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_pack0).count();
    if (pipelined) {
        HIPCHK(ctx, hipEventRecord(as.uploaded, ctx->h2d_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, as.uploaded, 0));
    }

    const int32_t n32 = (int32_t)n;
    gg_batch b = single_cloud_batch(ctx, slot, dev.d_pts, &n32, origin, &base_z, tf);
    as.h_labels = reinterpret_cast<uint8_t *>(as.h_index + n);
    const bool direct = ctx->results_direct != 0 && as.hd_counts != nullptr;
    int32_t *const res_counts = direct ? as.hd_counts : dev.d_counts, *const res_index = direct ? as.hd_counts + 16 : dev.d_index;
    b.d_labels = reinterpret_cast<uint8_t *>(res_index); // (+ label_shift = 4 n on the device: the launch's arguments do not depend on n)
    ctx->next_label_shift = (int)(n * 4);
    b.d_out_index = res_index;
    b.d_out_counts = res_counts;
    const int rc = enqueue_batch(ctx, &b, ctx->stream, plan);
    ctx->next_label_shift = 0;
    if (rc != GG_OK) return rc;
    if (direct) {
        HIPCHK(ctx, hipEventRecord(as.downloaded, ctx->stream)); // (the results are in host memory when k_label is done)
    } else {
        // results come back on their own stream, so that the next ticket's kernels do not queue behind this download
        const hipStream_t down = pipelined ? ctx->d2h_stream : ctx->stream;
        if (pipelined) {
            HIPCHK(ctx, hipEventRecord(as.computed, ctx->stream));
            HIPCHK(ctx, hipStreamWaitEvent(down, as.computed, 0));
        }
        HIPCHK(ctx, hipMemcpyAsync(as.h_counts, dev.d_counts, 64 + n * 5, hipMemcpyDeviceToHost, down)); // counts + index + labels: one copy
        HIPCHK(ctx, hipEventRecord(as.downloaded, down));
    }
    if (plan && (plan->mask & ~EARLY_LAYERS)) { // the layers that are only final now (ground, groundpatch, points) follow the results: the host
        Arena a = ctx->arena;                   // assembles the returned cloud while they travel
        enqueue_layer_downloads(ctx, a, slot, plan->mask & ~EARLY_LAYERS, *plan, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    }
    if (plan) HIPCHK(ctx, hipEventRecord(ctx->layers_event, ctx->stream));

    as.cloud = cloud;
    as.n = n;
    as.has_tf = tf != nullptr;
    if (tf) memcpy(as.tf, tf, sizeof as.tf);
    as.ticket = ctx->next_ticket;
    *ticket = ctx->next_ticket++;
    if (host_timing) ctx->host_t[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_pack0).count();
    return GG_OK;
}

int gg_filter_cloud_async(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *tf, const float origin[3],
                          double base_z, int *ticket)
{
    return enqueue_ticket(ctx, slot, cloud, n, tf, origin, base_z, ticket, true);
}

int gg_filter_cloud_wait(gg_context *ctx, int ticket, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label, int32_t *out_index)
{
    if (!ctx) return GG_ERR_INVALID;
    if (ticket != ctx->oldest_ticket || ticket >= ctx->next_ticket) return fail(ctx, GG_ERR_INVALID, "tickets are waited for in issue order");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    gg_context::AsyncSlot &as = ctx->async_slot[ctx->slot_of_ticket[ticket % GG_ASYNC_DEPTH]];
    ctx->oldest_ticket = ticket + 1; // (also on error below: the slot is reusable either way)
    static const bool host_timing = getenv("GG_HOST_TIMING") != nullptr;
    const auto t_w0 = std::chrono::steady_clock::now();
    SYNCCHK(ctx, hipEventSynchronize(as.downloaded));
    const auto t_w1 = std::chrono::steady_clock::now();
    const size_t n = as.n;
    if (out_n) *out_n = (size_t)as.h_counts[0];
    if (n && (out_label || out_index || out_cloud)) {
        // the returned cloud (:173-189): the host owns the input, so it assembles the output from index + label -- every input point has
        // its own position in the returned cloud (the pieces of the input write disjoint records); labels and index are copied out by
        // the same threads
        const gg_point32 *cloud = as.cloud;
        const double *tf = as.has_tf ? as.tf : nullptr;
        const int32_t *h_index = as.h_index;
        const uint8_t *h_labels = as.h_labels;
        ctx->helper.split(n, [&](size_t i0, size_t i1) {
            if (out_label) memcpy(out_label + i0, h_labels + i0, i1 - i0);
            if (out_index) memcpy(out_index + i0, h_index + i0, (i1 - i0) * 4);
            if (out_cloud) assemble_returned_cloud(cloud, h_index, h_labels, tf, out_cloud, i0, i1);
        });
    }
    if (host_timing) {
        ctx->host_t[2] += std::chrono::duration<double>(t_w1 - t_w0).count();
        ctx->host_t[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_w1).count();
        if (++ctx->host_calls % 256 == 0) {
            fprintf(stderr, "gg host path, ms per call: pack+upload calls %.3f, whole enqueue %.3f, wait %.3f, copy-out + assemble %.3f\n",
                    1e3 * ctx->host_t[0] / 256, 1e3 * ctx->host_t[1] / 256, 1e3 * ctx->host_t[2] / 256, 1e3 * ctx->host_t[3] / 256);
            ctx->host_t[0] = ctx->host_t[1] = ctx->host_t[2] = ctx->host_t[3] = 0.0;
        }
    }
    return GG_OK;
}

// the synchronous reference-shaped call = one ticket, waited for at once
static int filter_cloud_impl(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *tf, const float origin[3],
                             double base_z, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label, int32_t *out_index)
{
    if (!ctx) return GG_ERR_INVALID;
    if (ctx->next_ticket != ctx->oldest_ticket) return fail(ctx, GG_ERR_INVALID, "gg_filter_cloud while async tickets are outstanding");
    int ticket = -1;
    const int rc = enqueue_ticket(ctx, slot, cloud, n, tf, origin, base_z, &ticket, false);
    if (rc != GG_OK) return rc;
    return gg_filter_cloud_wait(ctx, ticket, out_cloud, out_n, out_label, out_index);
}

int gg_filter_cloud(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const float origin[3], double base_z,
                    gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label, int32_t *out_index)
{
    return filter_cloud_impl(ctx, slot, cloud, n, nullptr, origin, base_z, out_cloud, out_n, out_label, out_index);
}

int gg_filter_cloud_tf(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double map_from_cloud[12],
                       const float origin[3], double base_z, gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label,
                       int32_t *out_index)
{
    if (!map_from_cloud) return GG_ERR_INVALID;
    return filter_cloud_impl(ctx, slot, cloud, n, map_from_cloud, origin, base_z, out_cloud, out_n, out_label, out_index);
}

// gg_filter_cloud + the layers the caller publishes, as one call (include/groundgrid_hip.h): the eight layers that are final after
// k_reduce are extracted and downloaded on a side branch while the stencil and the sweep run, the other three follow the results
static bool host_range_registered(const gg_context *ctx, const void *p, size_t bytes)
{
    const char *c = static_cast<const char *>(p);
    for (const auto &r : ctx->registered)
        if (c >= r.first && c + bytes <= r.first + r.second) return true;
    return false;
}

int gg_host_register(gg_context *ctx, void *ptr, size_t bytes)
{
    if (!ctx || !ptr || !bytes) return GG_ERR_INVALID;
    if (host_range_registered(ctx, ptr, bytes)) return GG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    ctx->registered.emplace_back(static_cast<char *>(ptr), bytes);
    return GG_OK;
}

int gg_host_unregister(gg_context *ctx, void *ptr)
{
    if (!ctx || !ptr) return GG_ERR_INVALID;
    for (auto it = ctx->registered.begin(); it != ctx->registered.end(); ++it)
        if (it->first == static_cast<char *>(ptr)) {
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (nothing in flight may still write into it)
            HIPCHK(ctx, hipStreamSynchronize(ctx->d2h_stream));
            drop_graphs(ctx);                               // (captured downloads name the range)
            HIPCHK(ctx, hipHostUnregister(ptr));
            ctx->registered.erase(it);
            return GG_OK;
        }
    return fail(ctx, GG_ERR_INVALID, "gg_host_unregister: not a registered range");
}

int gg_filter_cloud_layers(gg_context *ctx, int slot, const gg_point32 *cloud, size_t n, const double *map_from_cloud, const float origin[3], double base_z,
                           gg_point32 *out_cloud, size_t *out_n, uint8_t *out_label, int32_t *out_index, float *const layers[GG_NUM_LAYERS])
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (ctx->next_ticket != ctx->oldest_ticket) return fail(ctx, GG_ERR_INVALID, "gg_filter_cloud_layers while async tickets are outstanding");
    unsigned mask = 0u;
    if (layers)
        for (int l = 0; l < GG_NUM_LAYERS; ++l)
            if (layers[l]) mask |= 1u << l;
    if (!mask || (ctx->flags & GG_FLAG_MINIMAL_LAYERS)) { // nothing to fuse / three layers are owed and computed on demand: one after the other
        const int rc = filter_cloud_impl(ctx, slot, cloud, n, map_from_cloud, origin, base_z, out_cloud, out_n, out_label, out_index);
        if (rc != GG_OK || !mask) return rc;
        void *d[GG_NUM_LAYERS];
        for (int l = 0; l < GG_NUM_LAYERS; ++l) d[l] = layers[l];
        return get_layers_impl(ctx, slot, d);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t C = (size_t)ctx->arena.g.C, plane = plane_floats(ctx);
    if (const int rc = ensure_plane_staging(ctx)) return rc;
    LayerPlan plan;
    plan.mask = mask;
    bool staged[GG_NUM_LAYERS] = {};
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!((mask >> l) & 1u)) continue;
        staged[l] = !host_range_registered(ctx, layers[l], C * sizeof(float));
        plan.dst[l] = staged[l] ? (void *)(ctx->h_planes + (size_t)l * plane) : (void *)layers[l];
    }
    int ticket = -1;
    const int rc = enqueue_ticket(ctx, slot, cloud, n, map_from_cloud, origin, base_z, &ticket, false, &plan);
    if (rc != GG_OK) {
        // the side branch may already copy into the caller's (registered) planes: nothing of this call is in flight when it returns
        (void)hipStreamSynchronize(ctx->d2h_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    // planes that came down into the staging block move on to the caller's: the early ones WHILE the device sweeps, the late ones at the end
    auto copy_staged = [&](unsigned group) {
        void *to[GG_NUM_LAYERS];
        int from[GG_NUM_LAYERS], n_want = 0;
        for (int l = 0; l < GG_NUM_LAYERS; ++l) {
            if (!staged[l] || !((group >> l) & 1u)) continue;
            to[n_want] = layers[l];
            from[n_want++] = l; // (layer l was staged in plane l)
        }
        copy_staged_planes(ctx, to, from, n_want, plane);
    };
    if (mask & EARLY_LAYERS) {
        HIPCHK(ctx, hipEventSynchronize(ctx->join_event)); // (the side branch: behind k_reduce, beside k_patch / k_sweep)
        copy_staged(EARLY_LAYERS);
    }
    const int rc_wait = gg_filter_cloud_wait(ctx, ticket, out_cloud, out_n, out_label, out_index); // (assembles the returned cloud while the late layers travel)
    SYNCCHK(ctx, hipEventSynchronize(ctx->layers_event));
    if (rc_wait != GG_OK) return rc_wait;
    if (ctx->layer_copy_failed) {
        ctx->layer_copy_failed = false;
        ctx->last_error = "gg_filter_cloud_layers: a layer download could not be enqueued";
        return GG_ERR_HIP;
    }
    copy_staged(~EARLY_LAYERS);
    return GG_OK;
}

// ---- RCCL, bound at run time (include/groundgrid_hip.h "the one collective of the path") --------------------------------
extern "C++" {
namespace {
struct Rccl {
    // the NCCL API as RCCL exports it (rccl.h): ncclResult_t == int, ncclSuccess == 0, ncclUint8 == 1, ncclComm_t / hipStream_t opaque
    struct UniqueId {
        char internal[128];
    };
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
    Rccl()
    {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(h, "ncclCommInitRank"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(h, "ncclAllGather"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        ok = GetUniqueId && CommInitRank && CommDestroy && AllGather;
    }
};
Rccl &rccl()
{
    static Rccl r; // (dlopen once, on first use)
    return r;
}
} // namespace
} // extern "C++"

int gg_collective_available(void) { return rccl().ok ? 1 : 0; }

int gg_comm_unique_id(uint8_t id_out[128])
{
    if (!id_out) return GG_ERR_INVALID;
    if (!rccl().ok) return GG_ERR_NO_DEVICE;
    Rccl::UniqueId id;
    if (rccl().GetUniqueId(&id) != 0) return GG_ERR_HIP;
    memcpy(id_out, id.internal, 128);
    return GG_OK;
}

int gg_comm_init_rank(const uint8_t id_in[128], int n_ranks, int rank, void **comm_out)
{
    if (!id_in || !comm_out || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return GG_ERR_INVALID;
    *comm_out = nullptr;
    if (!rccl().ok) return GG_ERR_NO_DEVICE;
    Rccl::UniqueId id;
    memcpy(id.internal, id_in, 128);
    if (rccl().CommInitRank(comm_out, n_ranks, id, rank) != 0) return GG_ERR_HIP;
    return GG_OK;
}

int gg_comm_init_rank_for(gg_context *ctx, const uint8_t id_in[128], int n_ranks, int rank, void **comm_out)
{
    if (!ctx) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = gg_comm_init_rank(id_in, n_ranks, rank, comm_out);
    if (rc != GG_OK) fail(ctx, rc, rc == GG_ERR_NO_DEVICE ? "librccl.so could not be loaded" : "ncclCommInitRank failed");
    return rc;
}

int gg_comm_destroy(void *comm)
{
    if (!comm) return GG_ERR_INVALID;
    if (!rccl().ok) return GG_ERR_NO_DEVICE;
    return rccl().CommDestroy(comm) == 0 ? GG_OK : GG_ERR_HIP;
}

int gg_allgather_label_masks(gg_context *ctx, void *comm, const uint8_t *d_send, uint8_t *d_recv, size_t bytes_per_rank, void *stream)
{
    if (!ctx) return GG_ERR_INVALID;
    if (!comm) return fail(ctx, GG_ERR_INVALID, "gg_allgather_label_masks: null communicator");
    if (!d_send || !d_recv || bytes_per_rank == 0) return fail(ctx, GG_ERR_INVALID, "gg_allgather_label_masks: null buffer / zero size");
    if (!rccl().ok) return fail(ctx, GG_ERR_NO_DEVICE, "librccl.so could not be loaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = pick_stream(ctx, stream);
    // the masks are written by the last batch: order the gather after it when it runs on another stream
    if (ctx->have_batch_event && ctx->last_batch_stream != s) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->batch_event, 0));
    if (const int rc_half = stream_waits_for_second_half(ctx, s)) return rc_half;
    const int rc = rccl().AllGather(d_send, d_recv, bytes_per_rank, /* ncclUint8 */ 1, comm, s);
    if (rc != 0) {
        char buf[256];
        snprintf(buf, sizeof buf, "ncclAllGather: %s", rccl().GetErrorString ? rccl().GetErrorString(rc) : "error");
        ctx->last_error = buf;
        return GG_ERR_HIP;
    }
    // a later batch on another stream that writes into the buffer this gather still reads must wait for it (enqueue_batch)
    HIPCHK(ctx, hipEventRecord(ctx->gather_event, s));
    ctx->gather_stream = s;
    ctx->gather_lo = d_send;
    ctx->gather_hi = d_send + bytes_per_rank;
    return GG_OK;
}

int gg_get_point_classes(gg_context *ctx, int slot, size_t n, uint8_t *out_class, int32_t *out_cell)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (n > ctx->max_points) return GG_ERR_CAPACITY;
    if (n == 0) return GG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    launch_decode_classes(ctx->arena, slot, n, ctx->d_stage_class, ctx->d_stage_cell, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    if (out_class) HIPCHK(ctx, hipMemcpyAsync(out_class, ctx->d_stage_class, n, hipMemcpyDeviceToHost, ctx->stream));
    if (out_cell) HIPCHK(ctx, hipMemcpyAsync(out_cell, ctx->d_stage_cell, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// The public stage members of the reference's class (include/groundgrid_hip.h "the stage members"), on the slot's layers as they stand.
int gg_run_stage(gg_context *ctx, int slot, int stage, const gg_stage_args *args)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!args) return fail(ctx, GG_ERR_INVALID, "gg_run_stage: null arguments");
    const Geometry &g = ctx->arena.g;
    switch (stage) {
    case GG_STAGE_DETECT_GROUND_PATCHES:
        if (args->section < -1 || args->section > 3) return fail(ctx, GG_ERR_INVALID, "gg_run_stage: section must be 0..3 or -1");
        break;
    case GG_STAGE_SPIRAL_GROUND_INTERPOLATION: break;
    case GG_STAGE_DETECT_GROUND_PATCH_3:
    case GG_STAGE_DETECT_GROUND_PATCH_5: {
        const int h = stage == GG_STAGE_DETECT_GROUND_PATCH_3 ? 1 : 2; // (the S x S blocks of :355 must stay inside the map: UB in the reference)
        if (args->i < h || args->j < h || args->i >= g.rows - h || args->j >= g.cols - h) return fail(ctx, GG_ERR_INVALID, "gg_run_stage: the cell's block leaves the map");
        break;
    }
    case GG_STAGE_INTERPOLATE_CELL:
        if (args->i < 1 || args->j < 1 || args->i >= g.rows - 1 || args->j >= g.cols - 1) return fail(ctx, GG_ERR_INVALID, "gg_run_stage: the cell's block leaves the map");
        break;
    default: return fail(ctx, GG_ERR_INVALID, "gg_run_stage: unknown stage");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    Arena a = ctx->arena;
    a.flags = ctx->flags;
    a.eigen_reduction = ctx->conv.eigen_reduction;
    const bool own = ctx->slot_own[slot] != 0;
    if (own) a.cfg = ctx->slot_dev[slot]; // (the single-cell stages read it by value; k_patch takes its SLOT_CFG variant below)
    if (stage == GG_STAGE_DETECT_GROUND_PATCHES || stage == GG_STAGE_SPIRAL_GROUND_INTERPOLATION) {
        // the many-cell stages are the path's own kernels: they take their slot and base_z from a parameter record like a batch of one
        int r;
        HIPCHK(ctx, ctx->ring.acquire(&r));
        CloudParams *hp = ctx->h_params + (size_t)r * ctx->n_slots, *dp = ctx->d_params + (size_t)r * ctx->n_slots;
        hp[0] = CloudParams{};
        hp[0].slot = slot;
        hp[0].base_z = (float)args->base_z;
        hp[0].pos_x = ctx->pos_x[slot];
        hp[0].pos_y = ctx->pos_y[slot];
        hp[0].cfg_index = own ? slot : -1;
        HIPCHK(ctx, hipMemcpyAsync(dp, hp, sizeof(CloudParams), hipMemcpyHostToDevice, s));
        if (stage == GG_STAGE_DETECT_GROUND_PATCHES) {
            a.slot_cfg_launch = own ? 1 : 0;
            launch_patch_stage(a, dp, slot, args->section, s);
        } else {
            sweep::Params sp = ctx->sweep_params;
            sp.decrease = own ? ctx->slot_cfg[slot].occupied_cells_decrease_factor : ctx->cfg.occupied_cells_decrease_factor;
            sp.inv_decrease = 1.0 / sp.decrease;
            sp.decay_fast = sp.decrease >= 1.25 && sp.decrease < 1e300;
            sp.keep_points = 1;
            launch_sweep(a, sp, dp, 1, s, nullptr);
        }
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, ctx->ring.recorded(r, s));
    } else {
        launch_stage_cell(a, slot, stage, args->i, args->j, s);
        HIPCHK(ctx, hipGetLastError());
    }
    ctx->no_confidence[slot] = 0; // (every stage may write confidences)
    ctx->gp_tainted[slot] = 1;    // (... from whatever the caller put into the layers)
    if (const int rc = own_stream_mutated_map(ctx)) return rc;
    SYNCCHK(ctx, hipStreamSynchronize(s));
    return GG_OK;
}

// GroundSegmentation::insert_cloud on the slot's map as it stands (include/groundgrid_hip.h): k_classify -> scan -> scatter on the range,
// then k_stage_insert continues the recurrences in the (densified) layers.
int gg_insert_cloud(gg_context *ctx, int slot, const gg_point32 *cloud, size_t start, size_t end, const float origin[3], uint8_t *out_class, int32_t *out_cell)
{
    if (!slot_ok(ctx, slot)) return GG_ERR_CAPACITY;
    if (!origin || end < start || (end > start && !cloud)) return fail(ctx, GG_ERR_INVALID, "gg_insert_cloud: null cloud / origin or end < start");
    const size_t n = end - start;
    if (n > ctx->max_points) return fail(ctx, GG_ERR_CAPACITY, "gg_insert_cloud: range larger than max_points");
    if (n == 0) return GG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = own_stream_waits_for_batches(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    // the per-call layers dense: the three lazily kept ones computed, the reset values written into the dead half columns
    if (const int rc = ensure_lazy_layers(ctx, slot, true)) return rc;
    Arena a = ctx->arena;
    a.flags = ctx->flags & ~(unsigned)GG_FLAG_MINIMAL_LAYERS;
    a.eigen_reduction = ctx->conv.eigen_reduction;
    if (ctx->slot_own[slot]) a.cfg = ctx->slot_dev[slot]; // (k_classify is the only kernel here that reads the configuration: by value)
    launch_materialise_maps(a, ctx->d_slot_maps + slot, 1, s);
    HIPCHK(ctx, hipGetLastError());
    for (size_t i = 0; i < n; ++i) {
        const gg_point32 &p = cloud[start + i];
        gg_point16 &d = ctx->h_stage_pts[i];
        d.x = p.x, d.y = p.y, d.z = p.z, d.ring = p.ring, d.pad = 0;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage_pts, ctx->h_stage_pts, n * sizeof(gg_point16), hipMemcpyHostToDevice, s));
    int r;
    HIPCHK(ctx, ctx->ring.acquire(&r));
    CloudParams *hp = ctx->h_params + (size_t)r * ctx->n_slots, *dp = ctx->d_params + (size_t)r * ctx->n_slots;
    hp[0] = CloudParams{};
    hp[0].slot = slot;
    hp[0].n_points = (int)n;
    hp[0].ox = origin[0], hp[0].oy = origin[1], hp[0].oz = origin[2];
    hp[0].pos_x = ctx->pos_x[slot];
    hp[0].pos_y = ctx->pos_y[slot];
    hp[0].no_confidence = ctx->no_confidence[slot] ? 1 : 0;
    hp[0].fresh = 0;
    HIPCHK(ctx, hipMemcpyAsync(dp, hp, sizeof(CloudParams), hipMemcpyHostToDevice, s));
    BatchIO io{};
    io.d_points = ctx->d_stage_pts;
    io.cloud_stride = ctx->max_points;
    io.point_format = GG_POINT16;
    const int front = launch_classify(a, dp, io, 1, (int)n, s);
    if (front == FRONT_THREE_LAUNCHES) launch_scan(a, dp, 1, s);
    if (front != FRONT_ONE_LAUNCH) launch_scatter(a, dp, 1, (int)n, s);
    launch_stage_insert(a, dp, s);
    // (k_scan dropped the liveness masks of the tiles this range left empty; their values are all still there: every half column holds its values)
    launch_fill_bytes((uint8_t *)(a.tile_live + (size_t)slot * a.tile_live_stride), (size_t)a.g.T * 4, 0xFF, s);
    launch_decode_classes(a, slot, n, ctx->d_stage_class, ctx->d_stage_cell, s);
    HIPCHK(ctx, hipGetLastError());
    if (out_class) HIPCHK(ctx, hipMemcpyAsync(out_class, ctx->d_stage_class, n, hipMemcpyDeviceToHost, s));
    if (out_cell) HIPCHK(ctx, hipMemcpyAsync(out_cell, ctx->d_stage_cell, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, ctx->ring.recorded(r, s));
    ctx->lazy_pending[slot] = 0; // (all nine layers are maintained and dense)
    if (const int rc = own_stream_mutated_map(ctx)) return rc;
    SYNCCHK(ctx, hipStreamSynchronize(s));
    return GG_OK;
}

// tools and tests only (not in the header): which path gg_cluster_planes takes.  value 1 = 32 x 32 tiles labelled in LDS first (k_region_tile +
// k_region_rim), 0 = k_region_seed + k_cluster_merge; the same results.  A negative value changes nothing.  Returns the path the library
// ships with (REGIONS_TILE_DEFAULT), GG_ERR_INVALID for a null context.
extern "C" int gg_debug_regions_tile(gg_context *ctx, int value)
{
    if (!ctx) return GG_ERR_INVALID;
    if (value >= 0) ctx->regions_tile = value ? 1 : 0;
    return REGIONS_TILE_DEFAULT;
}

// tools and tests only (not in the header): override the launch geometry the library would pick from the batch size (0 = back
// to the default).  key: "sweep_waves", "k2_per_cloud", "k2_dense_share".  Returns the chunk size PW for key "pw" (read-only:
// the arena is carved for it at gg_create; set GG_PW in the environment before gg_create to change it).
extern "C" int gg_debug_set_tuning(gg_context *ctx, const char *key, int value)
{
    if (!ctx || !key || value < 0) return GG_ERR_INVALID;
    if (!strcmp(key, "pw")) return ctx->arena.PW;
    if (!strcmp(key, "graph_replays")) return (int)std::min<long>(ctx->graph_replays, 1 << 30); // (read-only: how many calls replayed a captured graph)
    if (!strcmp(key, "fresh_count")) { // (read-only: how many maps are fresh -- gg_reset_maps left their layer unwritten and nothing has filled it since)
        int c = 0;
        for (int k = 0; k < ctx->n_slots; ++k) c += ctx->fresh[k] ? 1 : 0;
        return c;
    }
    if (!strcmp(key, "lazy_count")) { // (read-only: how many maps still owe the three lazily kept layers of their last cloud)
        int c = 0;
        for (int k = 0; k < ctx->n_slots; ++k) c += ctx->lazy_pending[k] ? 1 : 0;
        return c;
    }
    if (!strcmp(key, "export_variant_default")) return EXPORT_VARIANT_DEFAULT; // (read-only: the kernel gg_export_layers ships with)
    if (!strcmp(key, "import_variant_default")) return IMPORT_VARIANT_DEFAULT; // (read-only: the kernel gg_import_layers ships with)
    if (!strcmp(key, "images_variant_default")) return IMAGES_VARIANT_DEFAULT; // (read-only: the kernels gg_export_images ships with)
    if (!strcmp(key, "graphs")) { // 0 = every call launches eagerly, 1 = one cloud per call replays a captured graph (the default)
        ctx->graphs_enabled = value != 0;
        drop_graphs(ctx);
        return GG_OK;
    }
    drop_graphs(ctx); // (every other key changes what the launchers pick)
    if (!strcmp(key, "sweep_waves")) ctx->arena.tune_sweep_waves = value;
    else if (!strcmp(key, "sweep_gpw")) ctx->arena.tune_sweep_gpw = value;
    else if (!strcmp(key, "sweep_split")) ctx->arena.tune_sweep_split = value;
    else if (!strcmp(key, "sweep_pair")) ctx->arena.tune_sweep_pair = value;
    else if (!strcmp(key, "sweep_pair_wgs")) ctx->arena.tune_sweep_pair_wgs = value;
    else if (!strcmp(key, "sweep_pair_waves")) ctx->arena.tune_sweep_pair_waves = value;
    else if (!strcmp(key, "fresh_maps")) ctx->fresh_enabled = value != 0;
    else if (!strcmp(key, "front")) ctx->arena.tune_front = std::min(value, 3);
    else if (!strcmp(key, "sweep_poll_cap")) ctx->arena.tune_sweep_poll_cap = value;
    else if (!strcmp(key, "scan_parts")) ctx->arena.tune_scan_parts = value;
    else if (!strcmp(key, "scan_poll_cap")) ctx->arena.tune_scan_poll_cap = value;
    else if (!strcmp(key, "upload_pieces")) ctx->upload_pieces = value;
    else if (!strcmp(key, "results_direct")) ctx->results_direct = value; // (A/B: 0 = results into HBM and a copy behind k_label, as before round 5)
    else if (!strcmp(key, "halves_min_clouds")) ctx->halves_min_clouds = std::max(2, value); // (tests: GG_FLAG_CONCURRENT_HALVES on small batches)
    else if (!strcmp(key, "move_chunk")) ctx->move_chunk_tune = value;
    else if (!strcmp(key, "export_variant")) ctx->export_variant = value ? 1 : 0; // (A/B: 1 = gg_export_layers gathers in destination order, k_export_gather)
    else if (!strcmp(key, "slopes_variant")) ctx->slopes_variant = value ? 1 : 0; // (A/B: 1 = gg_export_slopes cell by cell, k_slopes_gather)
    else if (!strcmp(key, "import_variant")) ctx->import_variant = value ? 1 : 0; // (A/B: 1 = gg_import_layers scatters in source order, k_import_scatter)
    else if (!strcmp(key, "images_variant")) ctx->images_variant = value ? 1 : 0; // (A/B: 1 = gg_export_images cell by cell, k11_images.hip)
    else if (!strcmp(key, "halves_no_fork")) ctx->probe_no_fork = value != 0; // (measurement only: the side stream does not wait for the caller's)
    else if (!strcmp(key, "scan_fault")) ctx->arena.tune_scan_fault = value;
    else if (!strcmp(key, "sweep_fault")) ctx->arena.tune_sweep_fault = value;
    else if (!strcmp(key, "probe_unordered_streams")) ctx->probe_unordered_streams = value != 0; // (tools/fill_overlap_probe.py: the CALLER orders its streams)
    else if (!strcmp(key, "clear_device_error")) *ctx->h_dev_error = 0u;
    else if (!strcmp(key, "k2_per_cloud")) ctx->arena.tune_k2_per_cloud = value;
    else if (!strcmp(key, "k2_dense_share")) ctx->arena.tune_k2_dense_share = std::min(value, 15);
    else return GG_ERR_INVALID;
    return GG_OK;
}

// tools only (not in the header): cycle counters written by the last sweep when GG_SWEEP_TIMING=1 was set at gg_create
extern "C" int gg_debug_sweep_timing(gg_context *ctx, unsigned long long out[64])
{
    if (!ctx || !out || !ctx->d_sweep_dbg) return GG_ERR_INVALID;
    if (hipMemcpy(out, ctx->d_sweep_dbg, 64 * 8, hipMemcpyDeviceToHost) != hipSuccess) return GG_ERR_HIP;
    return GG_OK;
}

// tools only: what the pair sweep's wavefronts of the last launch's cloud 0 recorded (GG_PAIR_TIMING=1 at gg_create; tools/pair_timing.py)
extern "C" int gg_debug_pair_timing(gg_context *ctx, unsigned long long out[2048])
{
    if (!ctx || !out || !ctx->arena.pair_dbg) return GG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GG_ERR_HIP;
    if (hipMemcpy(out, ctx->arena.pair_dbg, 2048 * 8, hipMemcpyDeviceToHost) != hipSuccess) return GG_ERR_HIP;
    return GG_OK;
}

// tools only: k_reduce's work-group census by CU (GG_K2_DEBUG=5): 1024 keys x 8 counters; reset != 0 re-arms it
extern "C" int gg_debug_k2_census(gg_context *ctx, unsigned long long *out, int reset)
{
    if (!ctx || !out || ctx->arena.k2_debug != 5) return GG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GG_ERR_HIP;
    if (hipMemcpy(out, ctx->arena.k2_dbg, 1024 * 8 * 8, hipMemcpyDeviceToHost) != hipSuccess) return GG_ERR_HIP;
    if (reset) {
        std::vector<unsigned long long> z(1024 * 8, 0ull);
        for (int k = 0; k < 1024; ++k) z[(size_t)k * 8 + 4] = ~0ull; // (first start: a minimum)
        if (hipMemcpy(ctx->arena.k2_dbg, z.data(), z.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return GG_ERR_HIP;
    }
    return GG_OK;
}

// tools only: k_reduce's per-work-group records (GG_K2_DEBUG=6): n x 4 words
extern "C" int gg_debug_k2_trace(gg_context *ctx, unsigned long long *out, int n)
{
    if (!ctx || !out || ctx->arena.k2_debug != 6 || n < 1 || n > 65536) return GG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GG_ERR_HIP;
    if (hipMemcpy(out, ctx->arena.k2_dbg, (size_t)n * 4 * 8, hipMemcpyDeviceToHost) != hipSuccess) return GG_ERR_HIP;
    return GG_OK;
}

// tools only: k_reduce's per-phase cycle sums (GG_K2_DEBUG=9); reset != 0 clears them
extern "C" int gg_debug_k2_phases(gg_context *ctx, unsigned long long out[64], int reset)
{
    if (!ctx || !out || ctx->arena.k2_debug != 9) return GG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GG_ERR_HIP;
    std::vector<unsigned long long> all((size_t)32768 * 32);
    if (hipMemcpy(all.data(), ctx->arena.k2_dbg, all.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return GG_ERR_HIP;
    for (int k = 0; k < 64; ++k) out[k] = 0;
    for (size_t wg = 0; wg < 32768; ++wg)
        for (int k = 0; k < 32; ++k) out[k] += all[wg * 32 + k];
    if (reset && hipMemset(ctx->arena.k2_dbg, 0, all.size() * 8) != hipSuccess) return GG_ERR_HIP;
    return GG_OK;
}

int gg_get_kernel_times(gg_context *ctx, double ms[GG_NUM_KERNELS], int64_t launches[GG_NUM_KERNELS], int reset)
{
    if (!ctx) return GG_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = drain_profile(ctx);
    if (rc != GG_OK) return rc;
    for (int k = 0; k < GG_NUM_KERNELS; ++k) {
        if (ms) ms[k] = ctx->k_ms[k];
        if (launches) launches[k] = ctx->k_launches[k];
        if (reset) {
            ctx->k_ms[k] = 0.0;
            ctx->k_launches[k] = 0;
        }
    }
    return GG_OK;
}

} // extern "C"
