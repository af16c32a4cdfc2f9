// K19 -- gg_route_planes: the NAVIGATION FUNCTION of MANY maps in device memory (include/groundgrid_hip.h): per cell the exact cost D of the
// cheapest admissible 4- or 8-connected path to the nearest goal over a caller-given cost plane, the next cell on that path, three counts
// per map and, from one start cell per map, the cell list of the path.  What a caller otherwise gets from a download, a graph, Dijkstra on
// the host and an upload, per map and per frame.  D is the unique fixed point of D(q) = min over admissible p of D(p) + s * w(p), D = 0 on
// the goals, so any order of relaxations that ends at the fixed point gives the same words: the kernel is free to choose one.
//
// Three launches, none of which waits for another work-group, and no host decision between them.
//   k_route_relax   ONE WORK-GROUP PER MAP, 256 threads; the map's d_dist plane is the working memory.  The plane is cut into tiles of
//                   ROUTE_TILE x ROUTE_TILE = 64 x 64 cells and the work-group keeps one byte per tile in LDS: "active".  First every cell
//                   becomes 0 (an unblocked goal) or GG_ROUTE_NONE and the tiles with a goal become active.  Then, round after round, it
//                   takes the active tiles in order.  A tile is loaded with a one-cell halo into LDS -- D and the clamped weight w, 0 on a
//                   blocked cell and beyond the map: 2 x 66 x 67 words, 35.4 KB -- and relaxed there until a whole sweep changes nothing;
//                   the cells that changed are written back, and a changed cell on the tile's rim activates the up to three tiles whose
//                   halo holds it.  The launch ends with a round that finds no active tile.
//                   A thread loads eighteen words of the region, in three batches of six per plane whose loads are all issued before the
//                   first is used (the kernel is a template on the presence of d_blocked and d_cost, so that no load stands under a
//                   run-time condition), keeps the words of d_dist in registers and writes back the cells that differ from them.
//                   A SWEEP is four directional passes at once, one per wavefront: wavefront 0 walks the tile's lines downwards with a
//                   lane per column, 1 upwards, 2 walks the columns to the right with a lane per line, 3 to the left.  All four relax the
//                   same LDS image in place (Gauss-Seidel: a step reads what the step before wrote, so one pass carries a value across the
//                   whole tile along its direction and along both diagonals that lean into it) with an LDS atomic min, so a word only ever
//                   falls and never loses an update to another wavefront.  A straight corridor of any length inside a tile costs one
//                   sweep, not one sweep per cell as with Jacobi.  The row pitch 67 is odd: a line and a column of the image both fall on
//                   distinct banks.
//                   Every stored word is the cost of a real chain of admissible steps (or NONE), so it is an upper bound of D; the sweep
//                   that changes nothing has read every cell of the tile after the last write, so the tile is at the fixed point for its
//                   halo.  A blocked cell and a cell beyond the map keep NONE for ever, and NONE + s * 0 never wins a min, so the four
//                   straight neighbours need no test; a diagonal needs its two side cells' w != 0 (no corner cutting).
//                   LOOP BOUNDS, all in the loop conditions: a sweep visits every cell, so after k sweeps every cell whose cheapest path
//                   inside the region has <= k steps is final: at most 64 * 64 sweeps change something.  After k rounds every cell of the
//                   map whose cheapest path has <= k steps is final (its successor was final a round earlier; in the same tile the visit
//                   that wrote the successor also settled the cell, in another tile that write activated the cell's tile): at most
//                   rows * cols rounds find an active tile.
//                   max_cost = R: a tentative value above R is not stored.  Every cell on a cheapest path of a cell with D <= R has a
//                   smaller D, so those cells end as with R = 0 and all others keep NONE.
//                   The entry point guarantees max(straight, diagonal) * cost_max * rows * cols <= 2^31 - 2: every true D fits, every
//                   stored word is <= 2^31 - 1 and one step is <= 2^31 - 2, so the unsigned sum of a stored word and a step cannot wrap.
//   k_route_next    grid (chunks of 256 cells, maps), only when d_next or d_counts is given: per cell the first direction, in the fixed order
//                   of the header in (row, col) terms, whose admissible step attains D(q) = D(p) + s * w(p) (route_step), from the final D;
//                   the counts by ballot, LDS and at most three integer atomic adds per work-group.
//   k_route_paths   one lane per map, only with starts: start, next(start), ... until D == 0, at most rows * cols steps (D falls by at
//                   least 1 per step, so no cell comes twice); it reads d_next where that was given and calls route_step where not.
// A plane is `ny` lines of `nx` contiguous words ((cols, rows) row-major, (rows, cols) column-major).  The neighbourhood and the step costs
// are their own transpose, so D needs no notion of `order`; only the direction ORDER of d_next does (route_step).
//
// Algorithmic bytes per cell: 4 read per given input plane (goals, blocked, cost) + 4 written (D) + 4 written (next): 20 with everything.
// The relaxation is not a streaming kernel: a tile visit moves up to 3 x 66 x 66 x 4 B in (D, blocked, cost) and up to 64 x 64 x 4 B out,
// and costs 64 steps x 4 wavefronts per sweep, each step up to 9 LDS reads of D, 9 of w, 8 multiplies and one LDS atomic per lane.  Work
// per map = tile visits x sweeps per visit, which the data decides (DESIGN.md K19 has the counts of the benchmark's maps).  One map runs on
// one CU; 1024 maps are 1024 work-groups, four resident per CU at 39.7 KB of LDS and 128 VGPRs.
#include "gg_device.h"

namespace gg {

constexpr int ROUTE_REGION = ROUTE_TILE + 2; // a tile and its halo
constexpr int ROUTE_PITCH = ROUTE_TILE + 3;  // words per line of the LDS image: odd
constexpr uint32_t ROUTE_NONE = (uint32_t)GG_ROUTE_NONE;
static_assert(ROUTE_TILE == 64, "a line of a tile is one wavefront");
static_assert(2 * ROUTE_REGION * ROUTE_PITCH * 4 + ROUTE_MAX_TILES <= 40 * 1024, "four work-groups per CU");

// the clamped weight of a cell of map `map`, 0 where it is blocked
GG_DEV uint32_t route_weight(const RouteArgs &x, int map, int cell)
{
    if (x.blocked && x.blocked[(size_t)map * x.blocked_stride + (size_t)cell] >= 0) return 0u;
    if (!x.cost) return 1u;
    return (uint32_t)min(max(x.cost[(size_t)map * x.cost_stride + (size_t)cell], 1), x.cost_max);
}

// ... from the two words, for the loops of k_route_relax that load a batch of words before the first is used: with the planes' presence known
// at compile time those loads stand under no condition (a load under a run-time select is waited for one by one)
GG_DEV uint32_t route_weight_of(int32_t blocked_word, int32_t cost_word, int cost_max)
{
    return blocked_word >= 0 ? 0u : (uint32_t)min(max(cost_word, 1), cost_max);
}

GG_DEV uint32_t route_lds(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

constexpr int ROUTE_INIT_UNROLL = 8;                                               // cells of a thread in flight while a plane is initialised
constexpr int ROUTE_PER_THREAD = (ROUTE_REGION * ROUTE_REGION + 255) / 256;        // words of a region per thread: 18
constexpr int ROUTE_LOAD_BATCH = 6;                                                // ... of which this many are in flight per plane
static_assert(ROUTE_PER_THREAD % ROUTE_LOAD_BATCH == 0, "a region is loaded in whole batches");

template <bool BLOCKED, bool COST> __global__ __launch_bounds__(256, 4) void k_route_relax(const RouteArgs x)
{
    __shared__ uint32_t D[ROUTE_REGION * ROUTE_PITCH];
    __shared__ uint32_t W[ROUTE_REGION * ROUTE_PITCH];
    __shared__ uint8_t active[ROUTE_MAX_TILES];
    const int map = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nx = x.nx, ny = x.ny, n_tiles = x.tiles_x * x.tiles_y, cells = nx * ny;
    int32_t *dist = x.dist + (size_t)map * x.plane_stride;
    const int32_t *goals = x.goals + (size_t)map * x.goal_stride;
    const int32_t *blocked = BLOCKED ? x.blocked + (size_t)map * x.blocked_stride : nullptr;
    const int32_t *cost = COST ? x.cost + (size_t)map * x.cost_stride : nullptr;

    for (int t = tid; t < n_tiles; t += 256) active[t] = 0;
    __syncthreads();
    for (int base = 0; base < cells; base += 256 * ROUTE_INIT_UNROLL) {
        int32_t g[ROUTE_INIT_UNROLL], b[ROUTE_INIT_UNROLL];
#pragma unroll
        for (int j = 0; j < ROUTE_INIT_UNROLL; ++j) { // (every load of the batch is issued before the first is used)
            const int cell = base + 256 * j + tid, at = cell < cells ? cell : 0;
            g[j] = goals[at];
            b[j] = BLOCKED ? blocked[at] : -1;
        }
#pragma unroll
        for (int j = 0; j < ROUTE_INIT_UNROLL; ++j) {
            const int cell = base + 256 * j + tid;
            if (cell >= cells) continue;
            const bool goal = (g[j] >= 0) & (b[j] < 0);
            dist[cell] = goal ? 0 : GG_ROUTE_NONE;
            if (goal) active[(cell / nx / ROUTE_TILE) * x.tiles_x + (cell % nx) / ROUTE_TILE] = 1;
        }
    }
    __syncthreads();

    for (int round = 0; round <= cells; ++round) { // (at most `cells` rounds find an active tile)
        bool any = false;
        for (int t = 0; t < n_tiles; ++t) {
            if (!active[t]) continue; // (the same in every thread: `active` is written between the barriers below only)
            any = true;
            const int tx = t % x.tiles_x, ty = t / x.tiles_x;
            const int x0 = tx * ROUTE_TILE, y0 = ty * ROUTE_TILE;
            __syncthreads(); // every thread has read active[t], and the image of the tile before
            if (tid == 0) active[t] = 0;
            uint32_t before[ROUTE_PER_THREAD]; // the words of d_dist this thread loaded: what the write-back compares with
#pragma unroll
            for (int j0 = 0; j0 < ROUTE_PER_THREAD; j0 += ROUTE_LOAD_BATCH) {
                int32_t d[ROUTE_LOAD_BATCH], b[ROUTE_LOAD_BATCH], c[ROUTE_LOAD_BATCH];
                bool in_map[ROUTE_LOAD_BATCH];
#pragma unroll
                for (int k = 0; k < ROUTE_LOAD_BATCH; ++k) { // (every load of the batch is issued before the first is used)
                    const int i = tid + 256 * (j0 + k), gx = x0 - 1 + i % ROUTE_REGION, gy = y0 - 1 + i / ROUTE_REGION;
                    in_map[k] = (i < ROUTE_REGION * ROUTE_REGION) & (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny);
                    const int at = in_map[k] ? gy * nx + gx : 0; // (a cell of the map in every lane)
                    d[k] = dist[at];
                    b[k] = BLOCKED ? blocked[at] : -1;
                    c[k] = COST ? cost[at] : 1;
                }
#pragma unroll
                for (int k = 0; k < ROUTE_LOAD_BATCH; ++k) {
                    const int i = tid + 256 * (j0 + k);
                    before[j0 + k] = in_map[k] ? (uint32_t)d[k] : ROUTE_NONE;
                    if (i < ROUTE_REGION * ROUTE_REGION) {
                        D[(i / ROUTE_REGION) * ROUTE_PITCH + i % ROUTE_REGION] = before[j0 + k];
                        W[(i / ROUTE_REGION) * ROUTE_PITCH + i % ROUTE_REGION] = in_map[k] ? route_weight_of(b[k], c[k], x.cost_max) : 0u;
                    }
                }
            }
            __syncthreads();
            // wavefronts 0, 1: a lane per column, down and up the lines; 2, 3: a lane per line, right and left along the columns
            const bool along_x = (wave & 2) != 0, backwards = (wave & 1) != 0;
            const int ex = min(ROUTE_TILE, nx - x0), ey = min(ROUTE_TILE, ny - y0); // the tile's cells inside the map
            const int steps = along_x ? ex : ey;
            for (int sweep = 0; sweep <= ROUTE_TILE * ROUTE_TILE; ++sweep) { // (at most 64 * 64 sweeps change something)
                bool changed = false;
                for (int step = 0; step < steps; ++step) {
                    const int k = backwards ? steps - 1 - step : step;
                    const int c = (1 + (along_x ? lane : k)) * ROUTE_PITCH + 1 + (along_x ? k : lane);
                    if (W[c] == 0u) continue; // blocked, or beyond the map (no cross-lane operation below)
                    const uint32_t w_l = W[c - 1], w_r = W[c + 1], w_u = W[c - ROUTE_PITCH], w_d = W[c + ROUTE_PITCH];
                    const uint32_t cur = route_lds(&D[c]);
                    uint32_t best = cur;
                    best = min(best, route_lds(&D[c - ROUTE_PITCH]) + x.straight * w_u);
                    best = min(best, route_lds(&D[c - 1]) + x.straight * w_l);
                    best = min(best, route_lds(&D[c + 1]) + x.straight * w_r);
                    best = min(best, route_lds(&D[c + ROUTE_PITCH]) + x.straight * w_d);
                    if (x.diagonals) {
                        if (w_u != 0u && w_l != 0u) best = min(best, route_lds(&D[c - ROUTE_PITCH - 1]) + x.diagonal * W[c - ROUTE_PITCH - 1]);
                        if (w_u != 0u && w_r != 0u) best = min(best, route_lds(&D[c - ROUTE_PITCH + 1]) + x.diagonal * W[c - ROUTE_PITCH + 1]);
                        if (w_d != 0u && w_l != 0u) best = min(best, route_lds(&D[c + ROUTE_PITCH - 1]) + x.diagonal * W[c + ROUTE_PITCH - 1]);
                        if (w_d != 0u && w_r != 0u) best = min(best, route_lds(&D[c + ROUTE_PITCH + 1]) + x.diagonal * W[c + ROUTE_PITCH + 1]);
                    }
                    if (best < cur && best <= x.reach) {
                        __hip_atomic_fetch_min(&D[c], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        changed = true;
                    }
                }
                if (!__syncthreads_or(changed)) break; // (the same in every thread)
            }
            // write back what changed; a changed cell on the rim is in the halo of up to three other tiles
#pragma unroll
            for (int j = 0; j < ROUTE_PER_THREAD; ++j) { // (the words of the load, the halo left out)
                const int i = tid + 256 * j, ly = i / ROUTE_REGION - 1, lx = i % ROUTE_REGION - 1; // the cell's place in the tile
                if (lx < 0 || lx >= ex || ly < 0 || ly >= ey) continue; // (ly < ey <= 64: i lies inside the region)
                const uint32_t v = D[(ly + 1) * ROUTE_PITCH + lx + 1];
                if (v == before[j]) continue;
                dist[(y0 + ly) * nx + x0 + lx] = (int32_t)v;
                const int ax = lx == 0 ? -1 : lx == ROUTE_TILE - 1 ? 1 : 0, ay = ly == 0 ? -1 : ly == ROUTE_TILE - 1 ? 1 : 0;
                const bool x_in = ax != 0 && tx + ax >= 0 && tx + ax < x.tiles_x, y_in = ay != 0 && ty + ay >= 0 && ty + ay < x.tiles_y;
                if (x_in) active[t + ax] = 1;
                if (y_in) active[t + ay * x.tiles_x] = 1;
                if (x_in && y_in) active[t + ay * x.tiles_x + ax] = 1;
            }
            __syncthreads(); // d_dist and `active` are written before the next tile is chosen and loaded
        }
        if (!any) break;
    }
}

// The successor of the reached cell (cx, cy) with 0 < D = d < NONE: the linear index of the first p, in the direction order (-1,0), (0,-1),
// (0,+1), (+1,0), (-1,-1), (-1,+1), (+1,-1), (+1,+1) of (row, col), whose step is admissible and attains d == D(p) + s * w(p); -1 if none does
// (which the fixed point excludes).  A line is a row when row_major and a column when not: (a, b) is (dy, dx) or (dx, dy).
GG_DEV int route_step(const RouteArgs &x, int map, const int32_t *dist, int cx, int cy, uint32_t d)
{
    const int n_dirs = x.diagonals ? 8 : 4;
    for (int k = 0; k < n_dirs; ++k) {
        const int a = k < 4 ? (k == 0 ? -1 : k == 3 ? 1 : 0) : (k < 6 ? -1 : 1);
        const int b = k < 4 ? (k == 1 ? -1 : k == 2 ? 1 : 0) : ((k & 1) ? 1 : -1);
        const int dx = x.row_major ? b : a, dy = x.row_major ? a : b;
        const int px = cx + dx, py = cy + dy;
        if (px < 0 || px >= x.nx || py < 0 || py >= x.ny) continue;
        const int p = py * x.nx + px;
        const uint32_t w = route_weight(x, map, p);
        if (w == 0u) continue;
        if (k >= 4 && (route_weight(x, map, cy * x.nx + px) == 0u || route_weight(x, map, py * x.nx + cx) == 0u)) continue;
        if ((uint32_t)dist[p] + (k < 4 ? x.straight : x.diagonal) * w == d) return p;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_route_next(const RouteArgs x)
{
    __shared__ uint32_t wave_counts[4][3];
    const int map = (int)blockIdx.y, lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int cell = (int)(blockIdx.x * 256u + threadIdx.x), cells = x.nx * x.ny;
    const int32_t *dist = x.dist + (size_t)map * x.plane_stride;
    const bool in_map = cell < cells;
    const uint32_t d = in_map ? (uint32_t)dist[cell] : ROUTE_NONE;
    if (x.next && in_map) {
        int next = d == ROUTE_NONE ? -1 : cell;
        if (d != ROUTE_NONE && d != 0u) next = route_step(x, map, dist, cell % x.nx, cell / x.nx, d);
        x.next[(size_t)map * x.plane_stride + (size_t)cell] = next;
    }
    if (!x.counts) return; // (uniform)
    const unsigned long long goals = __ballot(in_map && d == 0u), reached = __ballot(in_map && d != ROUTE_NONE);
    // (a reached cell is not blocked: only the others are looked up)
    const unsigned long long open = __ballot(in_map && (d != ROUTE_NONE || route_weight(x, map, cell) != 0u));
    if (lane == 0) {
        wave_counts[wave][0] = (uint32_t)__popcll(goals);
        wave_counts[wave][1] = (uint32_t)__popcll(reached);
        wave_counts[wave][2] = (uint32_t)__popcll(open);
    }
    __syncthreads();
    if (threadIdx.x >= 3u) return;
    const int k = (int)threadIdx.x;
    const int sum = (int)(wave_counts[0][k] + wave_counts[1][k] + wave_counts[2][k] + wave_counts[3][k]);
    if (sum) atomicAdd(x.counts + (size_t)map * 3 + k, sum);
}

__global__ __launch_bounds__(64) void k_route_paths(const RouteArgs x, int n_maps)
{
    const int map = (int)(blockIdx.x * 64u + threadIdx.x);
    if (map >= n_maps) return;
    const int cells = x.nx * x.ny;
    const int32_t *dist = x.dist + (size_t)map * x.plane_stride;
    const int32_t *next = x.next ? x.next + (size_t)map * x.plane_stride : nullptr;
    int32_t *row = x.paths + (size_t)map * (size_t)x.max_path;
    int cell = x.starts[map], len = 0; // (the entry point checked -1 <= start < cells)
    if (cell >= 0 && (uint32_t)dist[cell] != ROUTE_NONE)
        for (int step = 0; step < cells && cell >= 0; ++step) { // (D falls at every step: no cell comes twice)
            if (len < x.max_path) row[len] = cell;
            ++len;
            const uint32_t d = (uint32_t)dist[cell];
            if (d == 0u) break;
            cell = next ? next[cell] : route_step(x, map, dist, cell % x.nx, cell / x.nx, d);
        }
    x.path_len[map] = len;
}

void launch_route(const RouteArgs &x, int n_maps, hipStream_t s)
{
    const auto relax = x.blocked ? (x.cost ? k_route_relax<true, true> : k_route_relax<true, false>) : (x.cost ? k_route_relax<false, true> : k_route_relax<false, false>);
    hipLaunchKernelGGL(relax, dim3(n_maps), dim3(256), 0, s, x);
    if (x.next || x.counts) {
        if (x.counts) (void)hipMemsetAsync(x.counts, 0, sizeof(int32_t) * 3 * (size_t)n_maps, s);
        hipLaunchKernelGGL(k_route_next, dim3((x.nx * x.ny + 255) / 256, n_maps), dim3(256), 0, s, x);
    }
    if (x.starts) hipLaunchKernelGGL(k_route_paths, dim3((n_maps + 63) / 64), dim3(64), 0, s, x, n_maps);
}

} // namespace gg
