// K15 -- gg_cluster_clouds: the obstacle CLUSTERS of MANY labelled clouds in device memory (include/groundgrid_hip.h): the connected
// components of the occupied cells of every cloud's obstacle grid as a plane of cluster ids, a table of the clusters and a cluster id per
// point.  What a caller composes today from gg_rasterize_clouds, a download, a connected-components pass per map on the host and an upload.
//
// The plane itself is the only working memory of the labelling (one 32-bit word per cell): first a counter, then a parent pointer of a
// union-find forest, then a rank, then the id.  The forest is lock-free and its ONLY write is atomicMin(parent[larger root], smaller root):
// a parent only ever decreases, so every chain is strictly descending (find takes at most rows * cols steps and a union, whose larger end
// strictly decreases from try to try, at most 2 * rows * cols tries), and the root of a finished component is its smallest cell index --
// which is what the numbering asks for.  A stale parent (these loads ask for no freshness beyond a launch boundary) is a former ancestor of
// the same component: it costs steps or a retry, because the atomic's return value is the truth, never a wrong union.  The forest itself
// (find, union, the runs of lanes that share an id) lives in cluster_core.h, and gg_cluster_planes (k26_regions.hip) drives the merge,
// flatten, scan and rank launches of this file on its own seeds: launch_cluster_forest, launch_cluster_ranks.
// Ten launches, all on the caller's buffers and one word per 256 cells of call scratch; L = the linear cell index of `order`:
//   k_cluster_cells<ZERO>     plane[L] := 0
//   k_cluster_points<COUNT>   the walk of cloud_walk.h; one atomic add per participating point into its cell
//   k_cluster_cells<SEED>     plane[L] := count >= min_points ? L : 0xFFFFFFFF
//   k_cluster_merge           every occupied cell is united with the occupied ones of the half of its neighbourhood that precedes it
//   k_cluster_flatten         plane[L] := find(L); the number of roots of every 256-cell chunk -> scratch
//   k_cluster_scan            one work-group per map: the chunks' counts become their exclusive prefix; d_n_clusters; the records
//                             k < min(K, max_clusters) take their initial words
//   k_cluster_rank            a root's rank = its chunk's prefix + the roots before it in the chunk (ballots); plane[root] := -(rank + 2),
//                             record.first_cell := root
//   k_cluster_apply           plane[L] := the rank behind plane[L] (a root decodes its own word, another cell the word of its root, which is
//                             the encoded or the decoded rank -- both read the same); cells and the four bounds of the records by integer
//                             atomics, reduced over the lanes of a wavefront that share an id first
//   k_cluster_points<IDS>     d_point_cluster; points and the height_key (cloud_walk.h) of the records, reduced likewise
//   k_cluster_finalise        a record's key becomes its float, or the quiet NaN 0x7FC00000
// No work-group waits for another, every loop is bounded by construction, no float is added and only integer atomics (add, min, max) are
// used: the outputs do not depend on scheduling.
//
// Algorithmic bytes: per input point and points launch 1 (labels; 0.25 with masks) + 16 (32: GG_POINT32), per participating point 8 gathered
// (the (ground, confidence) pair: only with a height band or a table) and one 4-byte atomic (COUNT) / 4 read + 4 written (IDS); per cell 4
// written by ZERO, 4 + 4 by SEED, 4 + 4 by the flatten, 4 + 4 by the apply, 4 read by the rank; per occupied cell the parents the merge
// walks; per cluster record 32 written and a handful of atomics per wavefront that touches it.
#include "cluster_core.h"
#include "region_args.h"

namespace gg {

// a cluster's record as eight words: cells, points, row_min, row_max, col_min, col_max, height_max (its key while the call runs), first_cell
GG_DEV uint32_t *cluster_record(const ClusterArgs &x, int io, int k) { return x.records + ((size_t)io * x.max_clusters + k) * 8; }

template <bool SEED>
__global__ __launch_bounds__(256) void k_cluster_cells(const Arena a, const ClusterArgs x)
{
    int cloud, chunk;
    cluster_cell_item(cloud, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    if (L >= a.g.C) return;
    uint32_t *p = x.planes + (size_t)cluster_io(x, cloud) * x.plane_stride + L;
    *p = SEED ? (*p >= (uint32_t)x.min_points ? (uint32_t)L : CLUSTER_EMPTY) : 0u;
}

// The plane as [majors][minors] words, L = major * minors + minor (row-major: major = row; column-major: major = column): 4- and
// 8-connectivity are symmetric under the transposition, so the neighbours that precede L are (major, minor - 1) and those of major - 1.
__global__ __launch_bounds__(256) void k_cluster_merge(const Arena a, const ClusterArgs x)
{
    int cloud, chunk;
    cluster_cell_item(cloud, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    if (L >= a.g.C) return;
    uint32_t *parent = x.planes + (size_t)cluster_io(x, cloud) * x.plane_stride;
    if (cluster_load(parent + L) == CLUSTER_EMPTY) return;
    const int minors = x.order == GG_PLANES_ROWMAJOR ? a.g.cols : a.g.rows;
    const int major = L / minors, minor = L - major * minors;
    const bool left = minor > 0 && cluster_load(parent + L - 1) != CLUSTER_EMPTY;
    const bool up = major > 0 && cluster_load(parent + L - minors) != CLUSTER_EMPTY;
    if (left) cluster_union(parent, (uint32_t)L, (uint32_t)(L - 1));
    if (up) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors));
    if (x.connectivity == 8 && major > 0 && !up) { // (with `up` occupied both diagonals hang on it through their own left / right unions)
        if (!left && minor > 0 && cluster_load(parent + L - minors - 1) != CLUSTER_EMPTY) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors - 1));
        if (minor + 1 < minors && cluster_load(parent + L - minors + 1) != CLUSTER_EMPTY) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors + 1));
    }
}

__global__ __launch_bounds__(256) void k_cluster_flatten(const Arena a, const ClusterArgs x)
{
    __shared__ uint32_t wave_roots[4];
    int cloud, chunk;
    cluster_cell_item(cloud, chunk);
    const int io = cluster_io(x, cloud);
    const int L = chunk * 256 + (int)threadIdx.x;
    uint32_t *parent = x.planes + (size_t)io * x.plane_stride;
    bool root = false;
    if (L < a.g.C && cluster_load(parent + L) != CLUSTER_EMPTY) {
        const uint32_t r = cluster_find(parent, (uint32_t)L);
        root = r == (uint32_t)L;
        if (!root) parent[L] = r; // (a walk that passes here meanwhile reads the old ancestor or the root)
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0) wave_roots[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) x.chunk_counts[(size_t)io * x.cell_chunks + chunk] = wave_roots[0] + wave_roots[1] + wave_roots[2] + wave_roots[3];
}

__global__ __launch_bounds__(256) void k_cluster_scan(const Arena a, const ClusterArgs x)
{
    __shared__ uint32_t sums[256];
    const int io = cluster_io(x, (int)blockIdx.x);
    uint32_t *counts = x.chunk_counts + (size_t)io * x.cell_chunks;
    const int t = (int)threadIdx.x;
    const int per = (x.cell_chunks + 255) / 256;
    const int q0 = min(t * per, x.cell_chunks), q1 = min(q0 + per, x.cell_chunks);
    uint32_t mine = 0u;
    for (int q = q0; q < q1; ++q) mine += counts[q];
    sums[t] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) { // inclusive scan over the 256 threads' sums
        const uint32_t v = t >= d ? sums[t - d] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    uint32_t at = sums[t] - mine;
    for (int q = q0; q < q1; ++q) {
        const uint32_t c = counts[q];
        counts[q] = at;
        at += c;
    }
    const int K = (int)sums[255];
    if (t == 0) x.n_clusters[io] = K;
    if (x.records)
        for (int k = t; k < min(K, x.max_clusters); k += 256) {
            uint32_t *w = cluster_record(x, io, k); // (single words: the caller's array need not be 16-byte aligned)
            w[0] = 0u;
            w[1] = 0u;
            w[2] = 0x7FFFFFFFu;
            w[3] = 0xFFFFFFFFu;
            w[4] = 0x7FFFFFFFu;
            w[5] = 0xFFFFFFFFu;
            w[6] = 0u;
            w[7] = 0xFFFFFFFFu;
        }
}

__global__ __launch_bounds__(256) void k_cluster_rank(const Arena a, const ClusterArgs x)
{
    __shared__ uint32_t wave_roots[4];
    int cloud, chunk;
    cluster_cell_item(cloud, chunk);
    const int io = cluster_io(x, cloud);
    const int L = chunk * 256 + (int)threadIdx.x;
    const int wave = threadIdx.x >> 6;
    uint32_t *plane = x.planes + (size_t)io * x.plane_stride;
    const bool root = L < a.g.C && plane[L] == (uint32_t)L;
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0) wave_roots[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!root) return;
    uint32_t rank = x.chunk_counts[(size_t)io * x.cell_chunks + chunk] + (uint32_t)rank_below(m);
    for (int w = 0; w < wave; ++w) rank += wave_roots[w];
    plane[L] = (uint32_t)(-(int)rank - 2);
    if (x.records && rank < (uint32_t)x.max_clusters) cluster_record(x, io, (int)rank)[7] = (uint32_t)L;
}

__global__ __launch_bounds__(256) void k_cluster_apply(const Arena a, const ClusterArgs x)
{
    int cloud, chunk;
    cluster_cell_item(cloud, chunk);
    const int io = cluster_io(x, cloud);
    const int L = chunk * 256 + (int)threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t *plane = x.planes + (size_t)io * x.plane_stride;
    int id = -1;
    if (L < a.g.C) {
        const int v = (int)cluster_load(plane + L);
        if (v <= -2) id = -v - 2; // a root: nobody else writes this word
        else if (v >= 0) {        // the index of its root, whose word is the encoded rank or, once the root's own thread was here, the rank
            const int w = (int)cluster_load(plane + v);
            id = w <= -2 ? -w - 2 : w;
        }
        if (id >= 0) plane[L] = (uint32_t)id;
    }
    if (!x.records) return; // (uniform)
    const int minors = x.order == GG_PLANES_ROWMAJOR ? a.g.cols : a.g.rows;
    const int major = L / minors, minor = L - major * minors;
    const int r = x.order == GG_PLANES_ROWMAJOR ? major : minor, c = x.order == GG_PLANES_ROWMAJOR ? minor : major;
    int rid = id < x.max_clusters ? id : -1;
    const auto send = [&](int to, int cells, int r_lo, int r_hi, int c_lo, int c_hi) GG_INLINE_LAMBDA {
        int *rec = reinterpret_cast<int *>(cluster_record(x, io, to));
        atomicAdd(rec + 0, cells);
        atomicMin(rec + 2, r_lo);
        atomicMax(rec + 3, r_hi);
        atomicMin(rec + 4, c_lo);
        atomicMax(rec + 5, c_hi);
    };
    cluster_id_runs(rid, lane, [&](int to, bool mine, int count, bool speaker) GG_INLINE_LAMBDA {
        const int r_lo = wave_min_i(mine ? r : 0x7FFFFFFF), r_hi = wave_max_i(mine ? r : -1);
        const int c_lo = wave_min_i(mine ? c : 0x7FFFFFFF), c_hi = wave_max_i(mine ? c : -1);
        if (speaker) send(to, count, r_lo, r_hi, c_lo, c_hi);
    });
    if (rid >= 0) send(rid, 1, r, r, c, c);
}

// IDS = false: the count launch.  IDS = true: the per-point ids and the records' points and height key.  NEED_H: the height of a point is
// computed (the band is not (-inf, +inf), or the table wants the largest)
template <int FMT, bool MASKS, bool NEED_H, bool IDS>
__global__ __launch_bounds__(256) void k_cluster_points(const Arena a, const ClusterArgs x)
{
    CloudChunk k;
    if (!cloud_chunk(a, x.cl, k) || k.base >= k.end) return; // (uniform over the wavefront; there is no barrier below)
    const int io = k.io;
    uint32_t *plane = x.planes + (size_t)io * x.plane_stride;
    int32_t *ids = IDS && x.point_cluster ? x.point_cluster + (size_t)io * x.cl.cloud_stride : nullptr;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    CloudFrame f;
    load_cloud_frame(a, x.cl.clouds[k.cloud], f);
    walk_chunk<FMT, MASKS, WALK_POINT>(x.cl, k, [&](int p, uint32_t sel, const uint4 &v, uint32_t) GG_INLINE_LAMBDA {
        int cell = -1; // the participating point's cell
        uint32_t key = 0u;
        if (sel == 2u) {
            float px = __uint_as_float(v.x), py = __uint_as_float(v.y), pz = __uint_as_float(v.z);
            int r, cc;
            if (locate_point(a, f, px, py, pz, r, cc)) {
                cell = linear_cell(a, row_major, r, cc);
                if (NEED_H) {
                    const float h = height_above_ground(a, f, pz, r, cc);
                    if (h < x.min_height || h > x.max_height) cell = -1; // (a NaN height participates)
                    else if (h == h) key = height_key(h);
                }
            }
        }
        if (!IDS) {
            if (cell >= 0) atomicAdd(plane + cell, 1u);
            return;
        }
        const int id = cell >= 0 ? (int)plane[cell] : -1; // (-1: its cell is not occupied)
        if (p < k.end && ids) ids[p] = id;
        if (!x.records) return; // (uniform: every lane is back for the ballots below)
        const auto send = [&](int to, uint32_t points, uint32_t top) GG_INLINE_LAMBDA {
            uint32_t *rec = cluster_record(x, io, to);
            atomicAdd(rec + 1, points);
            if (top) atomicMax(rec + 6, top);
        };
        int rid = id < x.max_clusters ? id : -1;
        cluster_id_runs(rid, k.lane, [&](int to, bool mine, int count, bool speaker) GG_INLINE_LAMBDA {
            const uint32_t top = wave_max_u(mine ? key : 0u);
            if (speaker) send(to, (uint32_t)count, top);
        });
        if (rid >= 0) send(rid, 1u, key);
    });
}

__global__ __launch_bounds__(256) void k_cluster_finalise(const ClusterArgs x, int n_clouds)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_clouds * x.max_clusters) return;
    const int io = (int)(i / x.max_clusters), k = (int)(i % x.max_clusters);
    if (k >= x.n_clusters[io]) return;
    uint32_t *w = cluster_record(x, io, k) + 6;
    *w = *w ? height_of_key(*w) : QUIET_NAN_BITS;
}

template <bool IDS> static void launch_cluster_points(const Arena &a, const ClusterArgs &x, bool need_h, int n_clouds, hipStream_t s)
{
    const dim3 grid((x.cl.nch + 3) / 4, n_clouds);
    dispatch_cloud_variant(x.cl, [&](auto fmt, auto masks) {
        constexpr int FMT = decltype(fmt)::value;
        constexpr bool MASKS = decltype(masks)::value;
        if (need_h) hipLaunchKernelGGL((k_cluster_points<FMT, MASKS, true, IDS>), grid, dim3(256), 0, s, a, x);
        else hipLaunchKernelGGL((k_cluster_points<FMT, MASKS, false, IDS>), grid, dim3(256), 0, s, a, x);
    });
}

static bool cluster_band(const ClusterArgs &x) { return !(x.min_height == -__builtin_inff() && x.max_height == __builtin_inff()); }

// THE occupancy of the clouds' obstacle grids, in x.planes: zero, count, seed.  gg_clearance_clouds (k16_clearance.hip) starts from it too:
// its occupied cells are those whose word is >= 0 as an int32, which is where d_cell_cluster >= 0 at the end of launch_cluster
void launch_cluster_occupancy(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s)
{
    const dim3 cells(x.cell_chunks, n_clouds);
    hipLaunchKernelGGL((k_cluster_cells<false>), cells, dim3(256), 0, s, a, x);
    launch_cluster_points<false>(a, x, cluster_band(x), n_clouds, s); // (the count gathers the ground only for a band)
    hipLaunchKernelGGL((k_cluster_cells<true>), cells, dim3(256), 0, s, a, x);
}

// merge, flatten: from x.planes[L] = occupied ? L : 0xFFFFFFFF to the root of every occupied cell, and the roots of every chunk in scratch
// (merge = false: the caller has united the cells itself)
void launch_cluster_forest(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s, bool merge)
{
    const dim3 cells(x.cell_chunks, n_clouds);
    if (merge) hipLaunchKernelGGL(k_cluster_merge, cells, dim3(256), 0, s, a, x);
    hipLaunchKernelGGL(k_cluster_flatten, cells, dim3(256), 0, s, a, x);
}

// scan, rank: from the roots of every chunk in scratch to x.n_clusters, the records' initial words and x.planes[root] = -(rank + 2)
void launch_cluster_ranks(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s)
{
    hipLaunchKernelGGL(k_cluster_scan, dim3(n_clouds), dim3(256), 0, s, a, x);
    hipLaunchKernelGGL(k_cluster_rank, dim3(x.cell_chunks, n_clouds), dim3(256), 0, s, a, x);
}

void launch_cluster(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s)
{
    const dim3 cells(x.cell_chunks, n_clouds);
    const bool band = cluster_band(x);
    launch_cluster_occupancy(a, x, n_clouds, s);
    launch_cluster_forest(a, x, n_clouds, s, true);
    launch_cluster_ranks(a, x, n_clouds, s);
    hipLaunchKernelGGL(k_cluster_apply, cells, dim3(256), 0, s, a, x);
    if (x.point_cluster || x.records) launch_cluster_points<true>(a, x, band || x.records != nullptr, n_clouds, s);
    if (x.records) {
        const size_t n_rec = (size_t)n_clouds * x.max_clusters;
        hipLaunchKernelGGL(k_cluster_finalise, dim3((uint32_t)((n_rec + 255) / 256)), dim3(256), 0, s, x, n_clouds);
    }
}

} // namespace gg
