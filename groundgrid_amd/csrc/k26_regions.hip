// K26 -- gg_cluster_planes: the connected REGIONS of any int32 plane of MANY maps in device memory (include/groundgrid_hip.h): the
// components of the cells whose word lies in [lo, hi], the small ones dropped, as a plane of region ids, a plane of component sizes, four
// counts per map and a table of 48-byte records with the centroid sums and the minimum of a second plane over every region.  What a caller
// composes today from a download, scipy.ndimage.label + bincount + a relabel per map on the host and an upload.
//
// The forest is K15's (cluster_core.h) and so are four of the launches (k15_cluster.hip launch_cluster_forest, launch_cluster_ranks), driven
// by a ClusterArgs without per-cloud records: the id plane is the working memory, a finished root is its component's smallest index, and
// the numbering by ascending smallest L comes from the ranks of the roots.  L = the linear cell index of `order`; per call:
//   k_region_tile             (RegionArgs::tile, the default) the seed and the unions inside 32 x 32 tiles, in LDS: plane[L] := the smallest L
//                             of the cell's component within its tile, or 0xFFFFFFFF; size[L] := 0; heads := 0
//   k_region_rim              ... the unions of k_cluster_merge across the tile borders, through global atomics
//   k_region_seed             (tile == 0, the A/B path) plane[L] := lo <= seeds[L] <= hi ? L : 0xFFFFFFFF; size[L] := 0; heads := 0, then
//   k_cluster_merge           (K15)
//   k_cluster_flatten         (K15) plane[L] := the root of L
//   k_region_sizes            size[root] += the lanes of a wavefront that share the root, one integer add per run of them      } only with
//   k_region_filter           size[L] := size[root]; a cell whose size is below min_cells becomes 0xFFFFFFFF -- behind the      } d_cell_size
//                             launch boundary after the merge, so no walk meets a hole --; the roots that are left are counted
//                             per 256-cell chunk (over the flatten's counts); heads: dropped components, member cells
//   k_cluster_scan, k_cluster_rank       (K15) the chunks' prefix, K -> scratch, plane[root] := -(rank + 2)
//   k_region_init             heads: K; the records k < min(K, max_regions) take their initial words
//   k_region_apply            plane[L] := the rank behind plane[L], as k_cluster_apply; heads: kept cells; the records' cells, bounds, 64-bit
//                             coordinate sums and the 64-bit minimum of (value ^ 0x80000000) << 32 | L, each reduced over the lanes of a
//                             wavefront that share an id first; first_cell by the root's own lane
//   k_region_finalise         the key's high word becomes value_min (the low word is value_cell already; the initial all-ones key reads
//                             INT32_MAX, -1)
// No work-group waits for another, every loop is bounded by construction, and only integer atomics that commute (add, min, max) are used:
// the outputs do not depend on scheduling.
//
// Algorithmic bytes per cell: 4 read + 4 written by the seed (+ 4 with sizes), 4 + 4 by the flatten, 4 read by the rank, 4 + 4 by the apply
// (+ 4 with values); with sizes 4 read by the size launch and 4 + 4 + 4 by the filter; per member cell the parents the merge walks; per
// region record 48 written and a handful of atomics per wavefront that touches it.
#include "cluster_core.h"
#include "region_args.h"

namespace gg {

// a region's record as twelve words: cells, row_min, row_max, col_min, col_max, first_cell, the key (value_cell, value_min), sum_row, sum_col
GG_DEV uint32_t *region_record(const RegionArgs &x, int io, int k) { return x.records + ((size_t)io * x.max_regions + k) * 12; }

GG_DEV unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_region_seed(const Arena a, const RegionArgs x)
{
    int map, chunk;
    cluster_cell_item(map, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    if (x.heads && chunk == 0 && threadIdx.x < 4) x.heads[(size_t)map * 4 + threadIdx.x] = 0;
    if (L >= a.g.C) return;
    const int w = x.seeds[(size_t)map * x.seed_stride + L];
    x.forest.planes[(size_t)map * x.forest.plane_stride + L] = w >= x.lo && w <= x.hi ? (uint32_t)L : CLUSTER_EMPTY;
    if (x.sizes) x.sizes[(size_t)map * x.size_stride + L] = 0u;
}

// The tile-local stage, in place of the seed and the merge: a work-group labels a REGION_TILE x REGION_TILE tile in LDS with the same
// descending-parent forest -- the local index l = ty * REGION_TILE + tx orders the cells of a tile as L does, so a tile root is the smallest
// L of its part of the component -- and writes each cell's tile root as its global parent.  k_region_rim then unites across the tile
// borders alone, through global atomics.  find in LDS takes at most 1024 steps.
constexpr int REGION_TILE = 32;
__global__ __launch_bounds__(256) void k_region_tile(const Arena a, const RegionArgs x)
{
    __shared__ uint32_t forest[REGION_TILE * REGION_TILE];
    int map, tile;
    cluster_cell_item(map, tile);
    const bool row_major = x.forest.order == GG_PLANES_ROWMAJOR;
    const int minors = row_major ? a.g.cols : a.g.rows, majors = row_major ? a.g.rows : a.g.cols;
    const int tiles_minor = (minors + REGION_TILE - 1) / REGION_TILE;
    const int m0 = tile / tiles_minor * REGION_TILE, n0 = tile % tiles_minor * REGION_TILE;
    if (x.heads && tile == 0 && threadIdx.x < 4) x.heads[(size_t)map * 4 + threadIdx.x] = 0;
    uint32_t *plane = x.forest.planes + (size_t)map * x.forest.plane_stride;
    unsigned member = 0u; // bit k: cell k * 256 + threadIdx.x of the tile is a member
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = k * 256 + (int)threadIdx.x, mj = m0 + (l >> 5), mn = n0 + (l & 31);
        bool is = false;
        if (mj < majors && mn < minors) {
            const int L = mj * minors + mn;
            const int w = x.seeds[(size_t)map * x.seed_stride + L];
            is = w >= x.lo && w <= x.hi;
            if (x.sizes) x.sizes[(size_t)map * x.size_stride + L] = 0u;
        }
        forest[l] = is ? (uint32_t)l : CLUSTER_EMPTY;
        member |= is ? 1u << k : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(member >> k & 1u)) continue;
        const int l = k * 256 + (int)threadIdx.x, ty = l >> 5, tx = l & 31;
        const bool left = tx > 0 && forest[l - 1] != CLUSTER_EMPTY; // (whether a word is empty never changes)
        const bool up = ty > 0 && forest[l - REGION_TILE] != CLUSTER_EMPTY;
        if (left) cluster_union(forest, (uint32_t)l, (uint32_t)(l - 1));
        if (up) cluster_union(forest, (uint32_t)l, (uint32_t)(l - REGION_TILE));
        if (x.forest.connectivity == 8 && ty > 0 && !up) {
            if (!left && tx > 0 && forest[l - REGION_TILE - 1] != CLUSTER_EMPTY) cluster_union(forest, (uint32_t)l, (uint32_t)(l - REGION_TILE - 1));
            if (tx + 1 < REGION_TILE && forest[l - REGION_TILE + 1] != CLUSTER_EMPTY) cluster_union(forest, (uint32_t)l, (uint32_t)(l - REGION_TILE + 1));
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = k * 256 + (int)threadIdx.x, mj = m0 + (l >> 5), mn = n0 + (l & 31);
        if (mj >= majors || mn >= minors) continue;
        uint32_t word = CLUSTER_EMPTY;
        if (member >> k & 1u) {
            const uint32_t r = cluster_find(forest, (uint32_t)l); // (nobody writes the forest any more)
            word = (uint32_t)((m0 + (int)(r >> 5)) * minors + n0 + (int)(r & 31));
        }
        plane[mj * minors + mn] = word;
    }
}

// behind k_region_tile: the unions of k_cluster_merge whose two cells lie in different tiles
__global__ __launch_bounds__(256) void k_region_rim(const Arena a, const RegionArgs x)
{
    int map, chunk;
    cluster_cell_item(map, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    if (L >= a.g.C) return;
    uint32_t *parent = x.forest.planes + (size_t)map * x.forest.plane_stride;
    const int minors = x.forest.order == GG_PLANES_ROWMAJOR ? a.g.cols : a.g.rows;
    const int major = L / minors, minor = L - major * minors;
    const bool top = major % REGION_TILE == 0, first = minor % REGION_TILE == 0, last = minor % REGION_TILE == REGION_TILE - 1;
    if (!(top || first || last)) return;
    if (cluster_load(parent + L) == CLUSTER_EMPTY) return;
    const bool left = minor > 0 && cluster_load(parent + L - 1) != CLUSTER_EMPTY;
    const bool up = major > 0 && cluster_load(parent + L - minors) != CLUSTER_EMPTY;
    if (left && first) cluster_union(parent, (uint32_t)L, (uint32_t)(L - 1));
    if (up && top) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors));
    if (x.forest.connectivity == 8 && major > 0 && !up) { // (the diagonals that k_cluster_merge takes, where they cross a tile border)
        if (!left && minor > 0 && (top || first) && cluster_load(parent + L - minors - 1) != CLUSTER_EMPTY) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors - 1));
        if (minor + 1 < minors && (top || last) && cluster_load(parent + L - minors + 1) != CLUSTER_EMPTY) cluster_union(parent, (uint32_t)L, (uint32_t)(L - minors + 1));
    }
}

// behind the flatten: plane[L] is the root of L (L itself on a root)
__global__ __launch_bounds__(256) void k_region_sizes(const Arena a, const RegionArgs x)
{
    int map, chunk;
    cluster_cell_item(map, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    uint32_t *size = x.sizes + (size_t)map * x.size_stride;
    int rid = -1; // (roots are cell indices: below 2^31)
    if (L < a.g.C) rid = (int)x.forest.planes[(size_t)map * x.forest.plane_stride + L]; // (0xFFFFFFFF reads -1)
    cluster_id_runs(rid, (int)(threadIdx.x & 63), [&](int to, bool, int count, bool speaker) GG_INLINE_LAMBDA {
        if (speaker) atomicAdd(size + to, (uint32_t)count);
    });
    if (rid >= 0) atomicAdd(size + rid, 1u);
}

__global__ __launch_bounds__(256) void k_region_filter(const Arena a, const RegionArgs x)
{
    __shared__ uint32_t wave_roots[4];
    int map, chunk;
    cluster_cell_item(map, chunk);
    const int L = chunk * 256 + (int)threadIdx.x;
    uint32_t *plane = x.forest.planes + (size_t)map * x.forest.plane_stride;
    uint32_t *size = x.sizes + (size_t)map * x.size_stride;
    bool member = false, root = false, dropped = false;
    if (L < a.g.C) {
        const uint32_t r = plane[L];
        member = r != CLUSTER_EMPTY;
        if (member) {
            root = r == (uint32_t)L;
            const uint32_t s = size[r]; // (a root's size word is written by nobody in this launch)
            if (!root) size[L] = s;
            dropped = s < (uint32_t)x.min_cells;
            if (dropped) plane[L] = CLUSTER_EMPTY; // (every lane reads its own plane word alone)
        }
    }
    const unsigned long long kept_roots = __ballot(root && !dropped), lost_roots = __ballot(root && dropped), members = __ballot(member);
    if ((threadIdx.x & 63) == 0) {
        wave_roots[threadIdx.x >> 6] = (uint32_t)__popcll(kept_roots);
        if (x.heads) {
            if (lost_roots) atomicAdd(x.heads + (size_t)map * 4 + 1, (int)__popcll(lost_roots));
            if (members) atomicAdd(x.heads + (size_t)map * 4 + 2, (int)__popcll(members));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) x.forest.chunk_counts[(size_t)map * x.forest.cell_chunks + chunk] = wave_roots[0] + wave_roots[1] + wave_roots[2] + wave_roots[3];
}

// grid (ceil(max(max_regions, 1) / 256), maps)
__global__ __launch_bounds__(256) void k_region_init(const RegionArgs x)
{
    const int map = (int)blockIdx.y, k = (int)(blockIdx.x * 256 + threadIdx.x);
    const int K = x.forest.n_clusters[map];
    if (k == 0 && x.heads) x.heads[(size_t)map * 4] = K;
    if (!x.records || k >= min(K, x.max_regions)) return;
    uint32_t *w = region_record(x, map, k); // (single words: the caller's array is 8-byte aligned, not more)
    w[0] = 0u;
    w[1] = 0x7FFFFFFFu;
    w[2] = 0xFFFFFFFFu;
    w[3] = 0x7FFFFFFFu;
    w[4] = 0xFFFFFFFFu;
    w[5] = 0xFFFFFFFFu;
    w[6] = 0xFFFFFFFFu;
    w[7] = 0xFFFFFFFFu;
    w[8] = w[9] = w[10] = w[11] = 0u;
}

// grid (ceil(rows * cols / REGION_APPLY_CELLS), maps), REGION_APPLY_CELLS threads: the interior of a large region fills whole work-groups,
// so the lanes of the work-group that hold its FIRST id are reduced over the wavefront, then over the work-group in LDS, and one lane
// sends one set of atomics for all of them; what is left goes the way of k_cluster_apply
constexpr int REGION_APPLY_CELLS = 1024;
constexpr int REGION_APPLY_WAVES = REGION_APPLY_CELLS / 64;
__global__ __launch_bounds__(REGION_APPLY_CELLS) void k_region_apply(const Arena a, const RegionArgs x)
{
    __shared__ int first_id[REGION_APPLY_WAVES];
    __shared__ int part[REGION_APPLY_WAVES][5];                // cells, r_lo, r_hi, c_lo, c_hi of a wavefront's lanes with the work-group's id
    __shared__ unsigned long long wide_part[REGION_APPLY_WAVES][3]; // sum_r, sum_c, key
    int map, chunk;
    cluster_cell_item(map, chunk);
    const int L = chunk * REGION_APPLY_CELLS + (int)threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *plane = x.forest.planes + (size_t)map * x.forest.plane_stride;
    int id = -1;
    bool root = false;
    if (L < a.g.C) {
        const int v = (int)cluster_load(plane + L);
        if (v <= -2) { // a root: nobody else writes this word
            id = -v - 2;
            root = true;
        } else if (v >= 0) { // the index of its root, whose word is the encoded rank or, once the root's own thread was here, the rank
            const int w = (int)cluster_load(plane + v);
            id = w <= -2 ? -w - 2 : w;
        }
        if (id >= 0) plane[L] = (uint32_t)id;
    }
    if (x.heads) { // (uniform)
        const unsigned long long kept = __ballot(id >= 0);
        if (lane == 0 && kept) {
            atomicAdd(x.heads + (size_t)map * 4 + 3, (int)__popcll(kept));
            if (!x.sizes) atomicAdd(x.heads + (size_t)map * 4 + 2, (int)__popcll(kept)); // (no filter ran: every member is kept)
        }
    }
    if (!x.records) return; // (uniform)
    const int minors = x.forest.order == GG_PLANES_ROWMAJOR ? a.g.cols : a.g.rows;
    const int major = L / minors, minor = L - major * minors;
    const int r = x.forest.order == GG_PLANES_ROWMAJOR ? major : minor, c = x.forest.order == GG_PLANES_ROWMAJOR ? minor : major;
    int rid = id < x.max_regions ? id : -1;
    if (root && rid >= 0) region_record(x, map, rid)[5] = (uint32_t)L;
    unsigned long long key = ~0ull;
    if (x.values && rid >= 0) key = ((unsigned long long)((uint32_t)x.values[(size_t)map * x.value_stride + L] ^ 0x80000000u) << 32) | (uint32_t)L;
    const auto send = [&](int to, int cells, int r_lo, int r_hi, int c_lo, int c_hi, unsigned long long sum_r, unsigned long long sum_c, unsigned long long k) GG_INLINE_LAMBDA {
        uint32_t *w = region_record(x, map, to);
        int *rec = reinterpret_cast<int *>(w);
        unsigned long long *wide = reinterpret_cast<unsigned long long *>(w); // [3] the key, [4] sum_row, [5] sum_col
        atomicAdd(rec + 0, cells);
        atomicMin(rec + 1, r_lo);
        atomicMax(rec + 2, r_hi);
        atomicMin(rec + 3, c_lo);
        atomicMax(rec + 4, c_hi);
        if (k != ~0ull) atomicMin(wide + 3, k);
        atomicAdd(wide + 4, sum_r);
        atomicAdd(wide + 5, sum_c);
    };
    { // the work-group's first id (every barrier below is reached by all its threads: nothing above returns on a lane's condition)
        const unsigned long long have = __ballot(rid >= 0);
        const int mine_first = __shfl(rid, have ? __ffsll((long long)have) - 1 : 0, 64);
        if (lane == 0) first_id[wave] = have ? mine_first : -1;
        __syncthreads();
        int bid = -1;
        for (int w = 0; w < REGION_APPLY_WAVES && bid < 0; ++w) bid = first_id[w];
        if (bid >= 0) { // (uniform over the work-group)
            const bool mine = rid == bid;
            const unsigned long long m = __ballot(mine);
            if (m) { // (uniform over the wavefront)
                const int r_lo = wave_min_i(mine ? r : 0x7FFFFFFF), r_hi = wave_max_i(mine ? r : -1);
                const int c_lo = wave_min_i(mine ? c : 0x7FFFFFFF), c_hi = wave_max_i(mine ? c : -1);
                const uint32_t sum_r = wave_sum(mine ? (uint32_t)r : 0u), sum_c = wave_sum(mine ? (uint32_t)c : 0u);
                const unsigned long long k = x.values ? wave_min_u64(mine ? key : ~0ull) : ~0ull;
                if (lane == 0) {
                    part[wave][1] = r_lo;
                    part[wave][2] = r_hi;
                    part[wave][3] = c_lo;
                    part[wave][4] = c_hi;
                    wide_part[wave][0] = sum_r;
                    wide_part[wave][1] = sum_c;
                    wide_part[wave][2] = k;
                }
            }
            if (lane == 0) part[wave][0] = (int)__popcll(m);
            if (mine) rid = -1;
            __syncthreads();
            if (threadIdx.x == 0) {
                int cells = 0, r_lo = 0x7FFFFFFF, r_hi = -1, c_lo = 0x7FFFFFFF, c_hi = -1;
                unsigned long long sum_r = 0ull, sum_c = 0ull, k = ~0ull;
                for (int w = 0; w < REGION_APPLY_WAVES; ++w) {
                    if (!part[w][0]) continue;
                    cells += part[w][0];
                    r_lo = min(r_lo, part[w][1]);
                    r_hi = max(r_hi, part[w][2]);
                    c_lo = min(c_lo, part[w][3]);
                    c_hi = max(c_hi, part[w][4]);
                    sum_r += wide_part[w][0];
                    sum_c += wide_part[w][1];
                    k = wide_part[w][2] < k ? wide_part[w][2] : k;
                }
                send(bid, cells, r_lo, r_hi, c_lo, c_hi, sum_r, sum_c, k);
            }
        }
    }
    cluster_id_runs(rid, lane, [&](int to, bool mine, int count, bool speaker) GG_INLINE_LAMBDA {
        const int r_lo = wave_min_i(mine ? r : 0x7FFFFFFF), r_hi = wave_max_i(mine ? r : -1);
        const int c_lo = wave_min_i(mine ? c : 0x7FFFFFFF), c_hi = wave_max_i(mine ? c : -1);
        const uint32_t sum_r = wave_sum(mine ? (uint32_t)r : 0u), sum_c = wave_sum(mine ? (uint32_t)c : 0u); // (64 coordinates: far below 2^32)
        const unsigned long long k = x.values ? wave_min_u64(mine ? key : ~0ull) : ~0ull;
        if (speaker) send(to, count, r_lo, r_hi, c_lo, c_hi, sum_r, sum_c, k);
    });
    if (rid >= 0) send(rid, 1, r, r, c, c, (unsigned long long)r, (unsigned long long)c, key);
}

__global__ __launch_bounds__(256) void k_region_finalise(const RegionArgs x)
{
    const int map = (int)blockIdx.y, k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= min(x.forest.n_clusters[map], x.max_regions)) return;
    region_record(x, map, k)[7] ^= 0x80000000u;
}

void launch_regions(const Arena &a, const RegionArgs &x, int n_maps, hipStream_t s)
{
    const dim3 cells(x.forest.cell_chunks, n_maps), table((uint32_t)((std::max(x.max_regions, 1) + 255) / 256), n_maps);
    if (x.tile) {
        const uint32_t tiles = (uint32_t)((a.g.rows + REGION_TILE - 1) / REGION_TILE) * (uint32_t)((a.g.cols + REGION_TILE - 1) / REGION_TILE);
        hipLaunchKernelGGL(k_region_tile, dim3(tiles, n_maps), dim3(256), 0, s, a, x);
        hipLaunchKernelGGL(k_region_rim, cells, dim3(256), 0, s, a, x);
    } else {
        hipLaunchKernelGGL(k_region_seed, cells, dim3(256), 0, s, a, x);
    }
    launch_cluster_forest(a, x.forest, n_maps, s, !x.tile);
    if (x.sizes) {
        hipLaunchKernelGGL(k_region_sizes, cells, dim3(256), 0, s, a, x);
        hipLaunchKernelGGL(k_region_filter, cells, dim3(256), 0, s, a, x);
    }
    launch_cluster_ranks(a, x.forest, n_maps, s);
    hipLaunchKernelGGL(k_region_init, table, dim3(256), 0, s, x);
    hipLaunchKernelGGL(k_region_apply, dim3((uint32_t)((a.g.C + REGION_APPLY_CELLS - 1) / REGION_APPLY_CELLS), n_maps), dim3(REGION_APPLY_CELLS), 0, s, a, x);
    if (x.records) hipLaunchKernelGGL(k_region_finalise, table, dim3(256), 0, s, x);
}

} // namespace gg
