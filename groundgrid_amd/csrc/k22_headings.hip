// K22 -- gg_route_headings: the NAVIGATION FUNCTION OF A STATE LATTICE for MANY maps in device memory (include/groundgrid_hip.h): per cell and
// per heading the exact cost D of the cheapest chain of motion primitives to a goal state, every state on the chain one the heading mask of
// gg_footprint_planes admits; the primitive to take, the best heading per cell, three counts per map and, from one start pose per map, the
// list of (cell, heading) pairs of the path.  What a caller otherwise gets from a download of the mask, a graph of (cell, heading) nodes,
// Dijkstra on the host and an upload.  D is the unique fixed point of D(k, q) = min over admissible moves m of D(k2, q + d) + s * w(q + d),
// D = 0 on the goal states, so any order of relaxations that ends at the fixed point gives the same words: the kernel is free to choose one.
//
// Three launches, none of which waits for another work-group, and no host decision between them.
//   k_headings_relax  ONE WORK-GROUP PER MAP, 512 threads; the map's K planes of d_dist are the working memory.  A plane is cut into tiles of
//                   T x T cells, T = 32 up to 16 headings and 16 above (a template parameter), and the work-group keeps one byte per tile in
//                   LDS: "active".  First every state becomes 0 (a goal state) or GG_ROUTE_NONE and the tiles with a goal state, and those
//                   whose halo holds one, become active (a goal state never changes, so no write-back would speak for it).  Then, round
//                   after round, it takes the active tiles in order.  A tile is loaded with a three-cell halo (the longest move) into LDS
//                   -- the K planes of D, the heading mask and the clamped weight w, mask and w 0 beyond the map:
//                   (K + 2) x (T + 6) x (T + 7) words, 106.7 KB at T = 32, K = 16, 68.8 KB at T = 16, K = 32, 59.3 KB at T = 32, K = 8 -- and
//                   relaxed there until a whole sweep changes nothing; the states that changed are written back, and a changed state within
//                   three cells of the tile's rim activates the up to three tiles whose halo holds it.  The launch ends with a round that
//                   finds no active tile.  LDS is dynamic and sized by the K of the call, so a call of few headings leaves room for a
//                   second work-group on the compute unit.
//                   Region loads stand under no run-time condition (the kernel is a template on the presence of d_cost): every thread loads
//                   from a clamped address, eight words of d_dist in flight before the first is used.  The write-back reads the tile's words
//                   of d_dist again and stores the states whose LDS word differs (K is a run-time value: a register copy of the loaded words
//                   would live in scratch); a visit whose first sweep changes nothing skips it.
//                   A SWEEP: the 512 threads are 512 / T slots of T lanes.  Slot j takes heading j mod K in variant j / K (slots beyond
//                   4 K idle): with 16 headings at T = 32 and 32 at T = 16 every heading has one slot, with 8 two, and so on.  A slot walks
//                   the T steps of the tile for its heading, a lane per position along a line stepping over the lines, or a lane per line
//                   stepping along the positions -- whichever axis the heading's first translating move is longer in -- and AGAINST that
//                   move: state (k, q) reads (k2, q + d), so the cell ahead is relaxed first and one pass carries a value across the whole
//                   tile along a straight run, as K19's directional passes do (Gauss-Seidel).  Odd variants walk the other way, variants 2
//                   and 3 along the other axis; a heading whose table has a translating move against the first (reverse moves) turns its
//                   direction round every other sweep, one with moves longer in the other axis swaps the axis every other pair of sweeps
//                   (the host decides both per heading: HeadingsArgs::walk).  All slots relax the same LDS image in place with an LDS atomic
//                   min, so a word only ever falls and never loses an update.  The pitch T + 7 is odd: a line and a column of the image
//                   both fall on distinct banks.  A step of a lane costs 2 + 2 x 8 LDS reads (mask, own D; D and w of the target of each of
//                   the 8 move slots, an absent move reading the own state at cost 0) and at most one LDS atomic; a sweep is T such steps
//                   per slot.  The moves of a slot's heading are decoded into registers once per visit.
//                   Every stored word is the cost of a real chain of admissible moves (or NONE), so it is an upper bound of D; an
//                   inadmissible state and every state beyond the map keeps NONE for ever (the source's mask bit is tested, and NONE +
//                   s * w never wins a min, so the target's needs no test).  The sweep that changes nothing has read every state of the
//                   tile after the last write, so the tile is at the fixed point for its halo.
//                   LOOP BOUNDS, all in the loop conditions: a sweep visits every state of the tile, so after j sweeps every state whose
//                   cheapest chain inside the region has <= j moves is final: at most K * T * T sweeps change something.  After j rounds
//                   every state of the map whose cheapest chain has <= j moves is final (its successor was final a round earlier; in the
//                   same tile the visit that wrote the successor also settled the state, in another tile that write activated the state's
//                   tile, whose halo holds the successor because no move is longer than three cells): at most K * rows * cols rounds find
//                   an active tile.
//                   max_cost = R: a tentative value above R is not stored.  Every state on a cheapest chain of a state with D <= R has a
//                   smaller D, so those states end as with R = 0 and all others keep NONE.
//                   The entry point guarantees max s * cost_max * rows * cols * K <= 2^31 - 2: every true D fits, every stored word is
//                   <= 2^31 - 1 and one move is <= 2^31 - 2, so the unsigned sum of a stored word and a move cannot wrap.
//   k_headings_next   grid (chunks of 256 cells, maps), only when d_next, d_best, d_best_heading or d_counts is given: per cell, heading by
//                   heading, the smallest move slot that attains D (headings_step), from the final D; the smallest heading with the least D;
//                   the counts by ballot, LDS and at most three integer atomic adds per work-group.
//   k_headings_paths  one lane per map, only with starts: (cell, heading), the state its move leads to, ... until D == 0, at most
//                   K * rows * cols steps (D falls by at least 1 per step, so no state comes twice); it reads d_next where that was given
//                   and calls headings_step where not.
// The entry point hands over the move table in (line, position) offsets, so nothing here knows the plane order.
#include "gg_device.h"

namespace gg {

constexpr uint32_t HEADINGS_NONE = (uint32_t)GG_ROUTE_NONE;
constexpr int HEADINGS_HALO = HEADINGS_MAX_STEP;
constexpr int HEADINGS_LOAD_BATCH = 8; // words of d_dist a thread has in flight

GG_DEV uint32_t headings_lds(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
GG_DEV uint32_t headings_weight_of(int32_t cost_word, int cost_max) { return (uint32_t)min(max(cost_word, 1), cost_max); }
GG_DEV uint32_t headings_bits(int K) { return K >= 32 ? 0xFFFFFFFFu : (1u << K) - 1u; }

// the dynamic LDS of k_headings_relax<T>: K planes of D, the mask, w, the packed table and a byte per tile
inline size_t headings_lds_bytes(int T, int K, int n_tiles)
{
    return ((size_t)(K + 2) * (T + 2 * HEADINGS_HALO) * (T + 2 * HEADINGS_HALO + 1) + (size_t)K * HEADINGS_MAX_MOVES) * sizeof(uint32_t) + (size_t)((n_tiles + 15) / 16 * 16);
}

// the tiles whose halo holds cell (gx, gy) become active -- up to three neighbours of its own tile -- and with `own` that tile too
template <int T> GG_DEV void headings_activate(uint8_t *active, int tiles_x, int tiles_y, int gx, int gy, bool own)
{
    const int tx = gx / T, ty = gy / T, lx = gx % T, ly = gy % T, t = ty * tiles_x + tx;
    const int ax = lx < HEADINGS_HALO ? -1 : lx >= T - HEADINGS_HALO ? 1 : 0, ay = ly < HEADINGS_HALO ? -1 : ly >= T - HEADINGS_HALO ? 1 : 0;
    const bool x_in = ax != 0 && tx + ax >= 0 && tx + ax < tiles_x, y_in = ay != 0 && ty + ay >= 0 && ty + ay < tiles_y;
    if (own) active[t] = 1;
    if (x_in) active[t + ax] = 1;
    if (y_in) active[t + ay * tiles_x] = 1;
    if (x_in && y_in) active[t + ay * tiles_x + ax] = 1;
}

template <int T, bool COST> __global__ __launch_bounds__(HEADINGS_THREADS) void k_headings_relax(const HeadingsArgs x)
{
    constexpr int THREADS = HEADINGS_THREADS, REGION = T + 2 * HEADINGS_HALO, PITCH = REGION + 1, PLANE = REGION * PITCH, R2 = REGION * REGION;
    constexpr int CELLS_PER_THREAD = (R2 + THREADS - 1) / THREADS;
    static_assert(PITCH % 2 == 1 && THREADS % T == 0, "an odd pitch, whole slots");
    extern __shared__ __attribute__((aligned(16))) uint32_t headings_smem[];
    const int K = x.n_headings, map = (int)blockIdx.x, tid = (int)threadIdx.x;
    uint32_t *D = headings_smem;                // [K][PLANE]
    uint32_t *M = D + (size_t)K * PLANE;        // [PLANE] heading mask, 0 beyond the map
    uint32_t *W = M + PLANE;                    // [PLANE] clamped weight, 0 beyond the map
    uint32_t *table = W + PLANE;                // [K][8]
    uint8_t *active = (uint8_t *)(table + K * HEADINGS_MAX_MOVES);
    const int nx = x.nx, ny = x.ny, n_tiles = x.tiles_x * x.tiles_y, cells = nx * ny;
    const uint32_t k_bits = headings_bits(K);
    int32_t *dist = x.dist + (size_t)map * x.dist_stride;
    const uint32_t *mask = x.mask + (size_t)map * x.mask_stride;
    const int32_t *goals = x.goals + (size_t)map * x.goal_stride;
    const int32_t *cost = COST ? x.cost + (size_t)map * x.cost_stride : nullptr;

    for (int t = tid; t < n_tiles; t += THREADS) active[t] = 0;
    for (int e = tid; e < K * HEADINGS_MAX_MOVES; e += THREADS) table[e] = x.table[e];
    __syncthreads();
    for (int base = 0; base < cells; base += THREADS * 4) {
        int32_t g[4];
        uint32_t m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { // (every load of the batch is issued before the first is used)
            const int cell = base + THREADS * j + tid, at = cell < cells ? cell : 0;
            g[j] = goals[at];
            m[j] = mask[at];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cell = base + THREADS * j + tid;
            if (cell >= cells) continue;
            const uint32_t goal_bits = g[j] >= 0 ? m[j] & x.goal_headings & k_bits : 0u;
            for (int k = 0; k < K; ++k) dist[(size_t)k * x.plane_stride + cell] = (goal_bits >> k) & 1u ? 0 : GG_ROUTE_NONE;
            // (a goal state never changes, so no write-back will speak for it: it activates its own tile and the tiles whose halo holds it)
            if (goal_bits) headings_activate<T>(active, x.tiles_x, x.tiles_y, cell % nx, cell / nx, true);
        }
    }
    __syncthreads();

    // this thread's slot: heading, variant and the heading's moves as offsets into the LDS image
    const int slot = tid / T, lane = tid % T, k_own = slot % K, variant = slot / K;
    const bool idle = variant >= 4;
    const uint32_t walk = x.walk[k_own];
    int d_off[HEADINGS_MAX_MOVES], w_off[HEADINGS_MAX_MOVES];
    uint32_t s_of[HEADINGS_MAX_MOVES];
#pragma unroll
    for (int m = 0; m < HEADINGS_MAX_MOVES; ++m) {
        const uint32_t u = table[k_own * HEADINGS_MAX_MOVES + m];
        s_of[m] = u >> 11;
        // (an absent move reads the own state at cost 0: it never wins the min)
        w_off[m] = s_of[m] ? ((int)(u & 7u) - HEADINGS_MAX_STEP) * PITCH + (int)((u >> 3) & 7u) - HEADINGS_MAX_STEP : 0;
        d_off[m] = (s_of[m] ? (int)((u >> 6) & 31u) : k_own) * PLANE + w_off[m];
    }

    for (int round = 0; round <= x.max_rounds; ++round) { // (at most K * cells rounds find an active tile)
        bool any = false;
        for (int t = 0; t < n_tiles; ++t) {
            if (!active[t]) continue; // (the same in every thread: `active` is written between the barriers below only)
            any = true;
            const int tx = t % x.tiles_x, ty = t / x.tiles_x;
            const int x0 = tx * T, y0 = ty * T;
            __syncthreads(); // every thread has read active[t], and the image of the tile before
            if (tid == 0) active[t] = 0;
            {
                uint32_t mw[CELLS_PER_THREAD];
                int32_t cw[CELLS_PER_THREAD];
                bool in_map[CELLS_PER_THREAD];
#pragma unroll
                for (int j = 0; j < CELLS_PER_THREAD; ++j) {
                    const int i = tid + THREADS * j, gx = x0 - HEADINGS_HALO + i % REGION, gy = y0 - HEADINGS_HALO + i / REGION;
                    in_map[j] = (i < R2) & (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny);
                    const int at = in_map[j] ? gy * nx + gx : 0; // (a cell of the map in every lane)
                    mw[j] = mask[at];
                    cw[j] = COST ? cost[at] : 1;
                }
#pragma unroll
                for (int j = 0; j < CELLS_PER_THREAD; ++j) {
                    const int i = tid + THREADS * j;
                    if (i >= R2) continue;
                    M[(i / REGION) * PITCH + i % REGION] = in_map[j] ? mw[j] & k_bits : 0u;
                    W[(i / REGION) * PITCH + i % REGION] = in_map[j] ? headings_weight_of(cw[j], x.cost_max) : 0u;
                }
            }
            for (int i0 = 0; i0 < K * R2; i0 += THREADS * HEADINGS_LOAD_BATCH) {
                int32_t d[HEADINGS_LOAD_BATCH];
                bool in_map[HEADINGS_LOAD_BATCH];
#pragma unroll
                for (int b = 0; b < HEADINGS_LOAD_BATCH; ++b) { // (every load of the batch is issued before the first is used)
                    const int i = min(i0 + THREADS * b + tid, K * R2 - 1), k = i / R2, c = i % R2;
                    const int gx = x0 - HEADINGS_HALO + c % REGION, gy = y0 - HEADINGS_HALO + c / REGION;
                    in_map[b] = (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny);
                    d[b] = dist[(size_t)k * x.plane_stride + (in_map[b] ? gy * nx + gx : 0)];
                }
#pragma unroll
                for (int b = 0; b < HEADINGS_LOAD_BATCH; ++b) {
                    const int i = i0 + THREADS * b + tid;
                    if (i >= K * R2) continue;
                    const int k = i / R2, c = i % R2;
                    D[k * PLANE + (c / REGION) * PITCH + c % REGION] = in_map[b] ? (uint32_t)d[b] : HEADINGS_NONE;
                }
            }
            __syncthreads();
            const int ex = min(T, nx - x0), ey = min(T, ny - y0); // the tile's cells inside the map
            int sweep = 0;
            for (; sweep <= x.max_sweeps; ++sweep) { // (at most K * T * T sweeps change something)
                bool changed = false;
                if (!idle) {
                    const int turn = variant + ((walk & HEADINGS_WALK_ALT_DIR) ? sweep & 1 : 0);
                    const int swap = (variant >> 1) + ((walk & HEADINGS_WALK_ALT_AXIS) ? (sweep >> 1) & 1 : 0);
                    const bool backwards = (((walk & HEADINGS_WALK_BACK) ? 1 : 0) + turn) & 1;
                    const bool along = (((walk & HEADINGS_WALK_POSITIONS) ? 1 : 0) + swap) & 1; // a lane per line, stepping along the positions
                    for (int step = 0; step < T; ++step) {
                        const int p = backwards ? T - 1 - step : step;
                        const int ly = along ? lane : p, lx = along ? p : lane;
                        if (ly >= ey || lx >= ex) continue; // beyond the map (no cross-lane operation below)
                        const int c = (ly + HEADINGS_HALO) * PITCH + lx + HEADINGS_HALO;
                        if (!((M[c] >> k_own) & 1u)) continue; // an inadmissible state keeps NONE
                        const uint32_t cur = headings_lds(&D[k_own * PLANE + c]);
                        uint32_t best = cur;
#pragma unroll
                        for (int m = 0; m < HEADINGS_MAX_MOVES; ++m) best = min(best, headings_lds(&D[d_off[m] + c]) + s_of[m] * W[w_off[m] + c]);
                        if (best < cur && best <= x.reach) {
                            __hip_atomic_fetch_min(&D[k_own * PLANE + c], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            changed = true;
                        }
                    }
                }
                if (!__syncthreads_or(changed)) break; // (the same in every thread)
            }
            // write back what changed; a changed state within the halo's width of the rim is in the halo of up to three other tiles
            if (sweep > 0) { // (uniform; the first sweep changed something)
                for (int i0 = 0; i0 < K * T * T; i0 += THREADS * HEADINGS_LOAD_BATCH) {
                    int32_t d[HEADINGS_LOAD_BATCH];
#pragma unroll
                    for (int b = 0; b < HEADINGS_LOAD_BATCH; ++b) { // (every load of the batch is issued before the first is used)
                        const int i = min(i0 + THREADS * b + tid, K * T * T - 1), k = i / (T * T), c = i % (T * T);
                        const int lx = min(c % T, ex - 1), ly = min(c / T, ey - 1);
                        d[b] = dist[(size_t)k * x.plane_stride + (y0 + ly) * nx + x0 + lx];
                    }
#pragma unroll
                    for (int b = 0; b < HEADINGS_LOAD_BATCH; ++b) {
                        const int i = i0 + THREADS * b + tid;
                        if (i >= K * T * T) continue;
                        const int k = i / (T * T), c = i % (T * T), lx = c % T, ly = c / T;
                        if (lx >= ex || ly >= ey) continue;
                        const uint32_t v = D[k * PLANE + (ly + HEADINGS_HALO) * PITCH + lx + HEADINGS_HALO];
                        if (v == (uint32_t)d[b]) continue;
                        dist[(size_t)k * x.plane_stride + (y0 + ly) * nx + x0 + lx] = (int32_t)v;
                        headings_activate<T>(active, x.tiles_x, x.tiles_y, x0 + lx, y0 + ly, false);
                    }
                }
            }
            __syncthreads(); // d_dist and `active` are written before the next tile is chosen and loaded
        }
        if (!any) break;
    }
}

// The move of the reached state (k, (cx, cy)) with 0 < D = d < NONE: the smallest slot m whose move attains d == D(k2, p) + s * w(p), -1 if
// none does (which the fixed point excludes).  An inadmissible target holds NONE and NONE + s * w is no D, so the mask is not looked up.
// *to receives the packed move.
GG_DEV int headings_step(const HeadingsArgs &x, const uint32_t *table, int map, const int32_t *dist, int k, int cx, int cy, uint32_t d, uint32_t *to)
{
    for (int m = 0; m < HEADINGS_MAX_MOVES; ++m) {
        const uint32_t u = table[k * HEADINGS_MAX_MOVES + m], s = u >> 11;
        if (!s) continue;
        const int py = cy + (int)(u & 7u) - HEADINGS_MAX_STEP, px = cx + (int)((u >> 3) & 7u) - HEADINGS_MAX_STEP, k2 = (int)((u >> 6) & 31u);
        if (px < 0 || px >= x.nx || py < 0 || py >= x.ny) continue;
        const int p = py * x.nx + px;
        const uint32_t w = x.cost ? headings_weight_of(x.cost[(size_t)map * x.cost_stride + (size_t)p], x.cost_max) : 1u;
        if ((uint32_t)dist[(size_t)k2 * x.plane_stride + p] + s * w == d) {
            *to = u;
            return m;
        }
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_headings_next(const HeadingsArgs x)
{
    __shared__ uint32_t table[HEADINGS_TABLE];
    __shared__ uint32_t wave_counts[4][3];
    const int K = x.n_headings, map = (int)blockIdx.y, lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int e = (int)threadIdx.x; e < K * HEADINGS_MAX_MOVES; e += 256) table[e] = x.table[e];
    __syncthreads();
    const int cell = (int)(blockIdx.x * 256u + threadIdx.x), cells = x.nx * x.ny;
    const bool in_map = cell < cells;
    const int at = in_map ? cell : 0;
    const int32_t *dist = x.dist + (size_t)map * x.dist_stride;
    const uint32_t admissible = in_map ? x.mask[(size_t)map * x.mask_stride + at] & headings_bits(K) : 0u;
    uint32_t best = HEADINGS_NONE, n_goal = 0, n_reached = 0, n_adm = 0;
    int best_heading = -1;
    for (int k = 0; k < K; ++k) { // (uniform)
        const uint32_t d = in_map ? (uint32_t)dist[(size_t)k * x.plane_stride + at] : HEADINGS_NONE;
        if (x.next && in_map) {
            int next = d == HEADINGS_NONE ? -1 : HEADINGS_AT_GOAL; // (every move costs >= 1: D == 0 on the goal states alone)
            uint32_t to;
            if (d != HEADINGS_NONE && d != 0u) next = headings_step(x, table, map, dist, k, cell % x.nx, cell / x.nx, d, &to);
            x.next[(size_t)map * x.next_stride + (size_t)k * x.next_plane_stride + cell] = next;
        }
        if (d < best) best = d, best_heading = k;
        n_goal += (uint32_t)__popcll(__ballot(in_map && d == 0u));
        n_reached += (uint32_t)__popcll(__ballot(in_map && d != HEADINGS_NONE));
        n_adm += (uint32_t)__popcll(__ballot((admissible >> k) & 1u));
    }
    if (in_map) {
        if (x.best) x.best[(size_t)map * x.best_stride + cell] = (int32_t)best;
        if (x.best_heading) x.best_heading[(size_t)map * x.best_heading_stride + cell] = best_heading;
    }
    if (!x.counts) return; // (uniform)
    if (lane == 0) {
        wave_counts[wave][0] = n_goal;
        wave_counts[wave][1] = n_reached;
        wave_counts[wave][2] = n_adm;
    }
    __syncthreads();
    if (threadIdx.x >= 3u) return;
    const int j = (int)threadIdx.x;
    const int sum = (int)(wave_counts[0][j] + wave_counts[1][j] + wave_counts[2][j] + wave_counts[3][j]);
    if (sum) atomicAdd(x.counts + (size_t)map * 3 + j, sum);
}

__global__ __launch_bounds__(64) void k_headings_paths(const HeadingsArgs x, int n_maps)
{
    const int map = (int)(blockIdx.x * 64u + threadIdx.x);
    if (map >= n_maps) return;
    const int32_t *dist = x.dist + (size_t)map * x.dist_stride;
    const int32_t *next = x.next ? x.next + (size_t)map * x.next_stride : nullptr;
    int32_t *row = x.paths + (size_t)map * x.path_stride;
    int cell = x.starts[map].x, k = x.starts[map].y, len = 0; // (the entry point checked -1 <= cell < cells and 0 <= heading < K)
    if (cell >= 0 && (uint32_t)dist[(size_t)k * x.plane_stride + cell] != HEADINGS_NONE)
        for (int step = 0; step <= x.max_rounds && cell >= 0; ++step) { // (D falls at every step: no state comes twice)
            if (len < x.max_len) row[2 * len] = cell, row[2 * len + 1] = k;
            ++len;
            const uint32_t d = (uint32_t)dist[(size_t)k * x.plane_stride + cell];
            if (d == 0u) break;
            uint32_t to = 0u;
            if (next) {
                const int m = next[(size_t)k * x.next_plane_stride + cell];
                to = m >= 0 && m < HEADINGS_MAX_MOVES ? x.table[k * HEADINGS_MAX_MOVES + m] : 0u;
            } else if (headings_step(x, x.table, map, dist, k, cell % x.nx, cell / x.nx, d, &to) < 0)
                to = 0u;
            if (!(to >> 11)) break; // (no move attains D: the fixed point excludes it)
            cell += ((int)(to & 7u) - HEADINGS_MAX_STEP) * x.nx + (int)((to >> 3) & 7u) - HEADINGS_MAX_STEP;
            k = (int)((to >> 6) & 31u);
        }
    x.path_len[map] = len;
}

template <int T> static void launch_headings_relax(const HeadingsArgs &x, int n_maps, hipStream_t s)
{
    const size_t lds = headings_lds_bytes(T, x.n_headings, x.tiles_x * x.tiles_y);
    static PerDeviceOnce big_lds;
    if (lds > 64 * 1024)
        big_lds.run([] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_headings_relax<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_headings_relax<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
        });
    if (x.cost) hipLaunchKernelGGL((k_headings_relax<T, true>), dim3(n_maps), dim3(HEADINGS_THREADS), lds, s, x);
    else hipLaunchKernelGGL((k_headings_relax<T, false>), dim3(n_maps), dim3(HEADINGS_THREADS), lds, s, x);
}

void launch_headings(const HeadingsArgs &x, int n_maps, hipStream_t s)
{
    if (x.tile == 32) launch_headings_relax<32>(x, n_maps, s);
    else launch_headings_relax<16>(x, n_maps, s);
    if (x.next || x.best || x.best_heading || x.counts) {
        if (x.counts) (void)hipMemsetAsync(x.counts, 0, sizeof(int32_t) * 3 * (size_t)n_maps, s);
        hipLaunchKernelGGL(k_headings_next, dim3((x.nx * x.ny + 255) / 256, n_maps), dim3(256), 0, s, x);
    }
    if (x.starts) hipLaunchKernelGGL(k_headings_paths, dim3((n_maps + 63) / 64), dim3(64), 0, s, x, n_maps);
}

} // namespace gg
