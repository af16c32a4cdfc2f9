// K20 -- gg_match_planes: CORRELATIVE SCAN-TO-MAP MATCHING of MANY maps in device memory (include/groundgrid_hip.h): the score S(k, dy, dx) of
// every yaw candidate k and every translation (dy, dx) of a (2 W + 1)^2 window -- the sum, over the scan cells of a map, of the clamped field
// word under the rotated, shifted and translated cell -- and the best candidate by the tie rule of the header, with the number of scan cells
// and the number of candidates that attain the best score.  What a caller composes today per map from nonzero (a synchronisation), a
// rotation, a scatter and a padded correlation per yaw.
//
// Two launches, nothing decided by the host in between, no work-group waits for another.
//   k_match_scores  one work-group per (map, group of up to MATCH_GROUP consecutive k), B = min(1024, candidates rounded up to 64) threads.
//                   Thread t owns the translations numbered t, t + B, ... (P = ceil((2 W + 1)^2 / B) <= 5 of them, a template parameter,
//                   so the accumulators are registers).  Translations are numbered along a line of the plane first: the lanes of a
//                   wavefront hold consecutive offsets along x, so one list entry makes a wavefront touch the few cache lines of
//                   ceil(64 / (2 W + 1)) + 1 line segments.
//                   The work-group walks the scan plane ONCE for all its k, in chunks of MATCH_CHUNK cells, coalesced; a ballot and a
//                   popcount per wavefront and one LDS add per wavefront append the linear indices of the chunk's scan cells to a list
//                   in LDS (the order of the list does not matter: the sums are integer).  When another chunk might not fit, or after the
//                   last one, the list is flushed, k by k: every entry is turned from a linear index into the field cell (x, y) under the
//                   rotated and shifted scan cell, packed into one word of a second list -- the division by the line length, the
//                   rotation and the rounding are paid per scan cell and k, not per cell of the plane -- and then every thread walks that
//                   list, reads an entry from LDS as a broadcast and makes one bounds-tested load of field[y + oy][x + ox] per
//                   translation it owns.  A cell whose whole window lies outside the map is stored as a far-away cell: its loads are
//                   predicated off, and such cells are few unless the shift empties the window.  The sums of a flush are added to the
//                   group's totals in LDS, each word by the one thread that owns it.
//                   At the end it writes, per k, the slice of the score volume if one is given, and a MatchPartial: the best key of this
//                   k, the number of translations of this k with that score, the scan cells of the map.
//   k_match_best    one wavefront per map: lane k reads the partial of k; the maximum key is the best candidate, the ties are those of the
//                   k whose best score equals it.
// The key is S in the high word and the complement of the packed tie rank (dy^2 + dx^2 | k | dy + W | dx + W: 12 + 6 + 7 + 7 bits) in the low
// word: S >= 0, so a plain unsigned 64-bit maximum applies "largest S, then smallest d2, k, dy, dx".  No global atomics.
// The group size depends on K and W alone (launch_match), never on the number of maps: one map and a thousand take the same path.
//
// Loop bounds: the chunk loop runs ceil(rows * cols / MATCH_CHUNK) times, the append loop MATCH_CHUNK / B times, the list never holds more
// than MATCH_LIST entries (it is flushed when fewer than MATCH_CHUNK are free), the list loops run to its length and the k loops to the
// group's size; the reductions are fixed.  Integers: |cq dr - sq dc| < 2^30 by rows, cols <= 32768 (the entry point checks), the rounded
// offset is < 2^17, the shift is clamped to a side, so every coordinate stays far inside an int32; a kept cell has -W <= x < nx + W, so
// x + 64 and y + 64 fit 16 bits each; an absent translation carries the offset -2^30, which no cell brings back into the map.
// S <= field_max * rows * cols <= 2^31 - 1 by the entry point's limit.
//
// Algorithmic work: scan cells * K * (2 W + 1)^2 field look-ups, most of them served by the L2 of the XCD the groups of a map share
// (xcd_contiguous_item), and ceil(K / group) reads of the scan plane.
#include "gg_device.h"

namespace gg {

constexpr int MATCH_CHUNK = 1024;        // cells of the scan plane a work-group looks at between two barriers
constexpr int MATCH_LIST = 2048;         // entries of either list in LDS (8 KiB each)
constexpr int MATCH_GROUP = 8;           // the most k of one work-group
constexpr int MATCH_TOTALS = 4608;       // words of LDS for the totals of a group: k of the group * translations (18 KiB)
constexpr int MATCH_MAX_THREADS = 1024;
constexpr int MATCH_MAX_PER_THREAD = 5;  // ceil(65 * 65 / 1024)
constexpr int MATCH_ABSENT = -(1 << 30); // the offset of a translation number beyond the window
constexpr int MATCH_BIAS = 64;           // added to x and y of a packed cell: > MATCH_MAX_WINDOW
constexpr uint32_t MATCH_DROPPED = 0xFFFFFFFFu; // a packed cell no translation brings inside (x = y = 65471 >= 32768 + 32)
static_assert(MATCH_CHUNK % 64 == 0 && MATCH_LIST >= 2 * MATCH_CHUNK, "whole wavefronts append, and a flushed list takes a chunk");
static_assert((2 * MATCH_MAX_WINDOW + 1) * (2 * MATCH_MAX_WINDOW + 1) <= MATCH_MAX_THREADS * MATCH_MAX_PER_THREAD, "every translation has a thread");
static_assert((2 * MATCH_MAX_WINDOW + 1) * (2 * MATCH_MAX_WINDOW + 1) <= MATCH_TOTALS, "the totals of one k fit");
static_assert(MATCH_BIAS > MATCH_MAX_WINDOW && 32768 + MATCH_MAX_WINDOW + MATCH_BIAS < 65535 - MATCH_BIAS - MATCH_MAX_WINDOW, "a packed coordinate fits 16 bits, and the dropped cell stays outside");
static_assert(MATCH_MAX_ROTATIONS <= 64, "k_match_best: one lane per k");

// round half away from zero of a Q14 value, the convention of gg_visibility_clouds
GG_DEV int match_round(int v)
{
    const int m = (abs(v) + 8192) >> 14;
    return v < 0 ? -m : m;
}

GG_DEV uint32_t match_rank(int k, int dy, int dx, int W)
{
    return (uint32_t)(dy * dy + dx * dx) << 20 | (uint32_t)k << 14 | (uint32_t)(dy + W) << 7 | (uint32_t)(dx + W);
}

GG_DEV unsigned long long match_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

GG_DEV uint32_t match_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

template <int P> __global__ __launch_bounds__(MATCH_MAX_THREADS) void k_match_scores(const MatchArgs x, int group, int n_groups)
{
    __shared__ int cells[MATCH_LIST];        // linear indices of scan cells
    __shared__ uint32_t under[MATCH_LIST];   // ... and, for the k at hand, the field cell under each: (x + 64) << 16 | (y + 64)
    __shared__ int totals[MATCH_TOTALS];     // [k of the group][translation]
    __shared__ int n_list;
    __shared__ unsigned long long wave_key[MATCH_MAX_THREADS / 64];
    __shared__ uint32_t wave_ties[MATCH_MAX_THREADS / 64], wave_cells[MATCH_MAX_THREADS / 64];
    const uint32_t it = xcd_contiguous_item(blockIdx.x, gridDim.x);
    const int map = (int)(it / (uint32_t)n_groups), k0 = (int)(it % (uint32_t)n_groups) * group, kn = min(group, x.n_rotations - k0);
    const int t = (int)threadIdx.x, B = (int)blockDim.x, lane = t & 63, wave = t >> 6, n_waves = B >> 6;
    const int W = x.window, D = 2 * W + 1, n_cand = D * D;
    const int nx = x.nx, ny = x.ny, C = nx * ny;
    const bool row_major = x.row_major;
    const int rows = row_major ? ny : nx, cols = row_major ? nx : ny;
    const int2 sh = x.shifts ? x.shifts[map] : make_int2(0, 0);               // (rows, cols), clamped by the entry point
    const int2 pv = x.pivots ? x.pivots[map] : make_int2(rows / 2, cols / 2); // (row, col)
    const int32_t *scan = x.scan + (size_t)map * x.scan_stride;
    const int32_t *field = x.field + (size_t)map * x.field_stride;

    // the translations of this thread as offsets (along a line, across lines)
    int ox[P], oy[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int j = t + p * B;
        oy[p] = j < n_cand ? j / D - W : MATCH_ABSENT;
        ox[p] = j < n_cand ? j % D - W : MATCH_ABSENT;
    }
    for (int j = t; j < kn * n_cand; j += B) totals[j] = 0; // (kn * n_cand <= MATCH_TOTALS: launch_match)
    if (t == 0) n_list = 0;
    __syncthreads();
    uint32_t my_cells = 0u;
    for (int base = 0; base < C; base += MATCH_CHUNK) {
        for (int i = t; i < MATCH_CHUNK; i += B) { // (whole wavefronts: B and MATCH_CHUNK are multiples of 64)
            const int cell = base + i;
            const bool is = cell < C && scan[cell] > 0;
            const unsigned long long m = __ballot(is);
            if (m == 0ull) continue; // (uniform over the wavefront)
            int at = 0;
            if (lane == 0) at = atomicAdd(&n_list, __popcll(m));
            at = __shfl(at, 0, 64) + rank_below(m);
            if (is) cells[at] = cell;
            my_cells += is;
        }
        __syncthreads();
        const int n = n_list;
        __syncthreads(); // (everyone has read n before anyone appends again or thread 0 resets it)
        if (n <= MATCH_LIST - MATCH_CHUNK && base + MATCH_CHUNK < C) continue; // (uniform: the next chunk still fits)
        if (t == 0) n_list = 0;
        for (int kk = 0; kk < kn; ++kk) {
            const int2 rot = x.rotations ? x.rotations[k0 + kk] : make_int2(16384, 0); // (cq, sq)
            for (int e = t; e < n; e += B) { // linear index -> the field cell under the rotated, shifted scan cell
                const int cell = cells[e], line = cell / nx, pos = cell - line * nx;
                const int dr = (row_major ? line : pos) - pv.x, dc = (row_major ? pos : line) - pv.y;
                const int fr = pv.x + match_round(rot.x * dr - rot.y * dc) + sh.x, fc = pv.y + match_round(rot.y * dr + rot.x * dc) + sh.y;
                const int fx = row_major ? fc : fr, fy = row_major ? fr : fc;
                const bool near = fx + W >= 0 && fx - W < nx && fy + W >= 0 && fy - W < ny; // some translation of the window lies inside
                under[e] = near ? (uint32_t)(fx + MATCH_BIAS) << 16 | (uint32_t)(fy + MATCH_BIAS) : MATCH_DROPPED;
            }
            __syncthreads();
            int acc[P];
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = 0;
#pragma unroll 4
            for (int e = 0; e < n; ++e) {
                const uint32_t b = under[e]; // (a broadcast)
                const int bx = (int)(b >> 16) - MATCH_BIAS, by = (int)(b & 0xFFFFu) - MATCH_BIAS;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int fx = bx + ox[p], fy = by + oy[p];
                    if ((unsigned)fx < (unsigned)nx && (unsigned)fy < (unsigned)ny) acc[p] += min(max(field[fy * nx + fx], 0), x.field_max);
                }
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (t + p * B < n_cand) totals[kk * n_cand + t + p * B] += acc[p]; // (this thread's word, and nobody else's)
            __syncthreads(); // (`under` is free for the next k, and after the last k `cells` for the next chunk)
        }
    }

    my_cells = match_wave_sum(my_cells); // (every lane is back here)
    if (lane == 0) wave_cells[wave] = my_cells;
    for (int kk = 0; kk < kn; ++kk) {
        const int k = k0 + kk;
        // the slice of the volume, and this thread's best key
        unsigned long long key = 0ull;
        int32_t *volume = x.scores ? x.scores + (size_t)map * x.score_stride + (size_t)k * (size_t)n_cand : nullptr;
        int S[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            S[p] = -1; // (no score)
            if (t + p * B >= n_cand) continue;
            S[p] = totals[kk * n_cand + t + p * B];
            const int dy = row_major ? oy[p] : ox[p], dx = row_major ? ox[p] : oy[p];
            if (volume) volume[(dy + W) * D + dx + W] = S[p];
            const unsigned long long mine = (unsigned long long)(uint32_t)S[p] << 32 | (unsigned long long)(~match_rank(k, dy, dx, W));
            key = mine > key ? mine : key;
        }
        key = match_wave_max(key); // (the translation (0, 0) exists, so the maximum over the work-group is a real key)
        if (lane == 0) wave_key[wave] = key;
        __syncthreads();
        for (int w = 0; w < n_waves; ++w) key = wave_key[w] > key ? wave_key[w] : key;
        const int best = (int)(key >> 32);
        uint32_t ties = 0u;
#pragma unroll
        for (int p = 0; p < P; ++p) ties += S[p] == best;
        ties = match_wave_sum(ties);
        if (lane == 0) wave_ties[wave] = ties;
        __syncthreads();
        if (t == 0) {
            uint32_t n_ties = 0u, n_cells = 0u;
            for (int w = 0; w < n_waves; ++w) {
                n_ties += wave_ties[w];
                n_cells += wave_cells[w];
            }
            x.partials[(size_t)map * MATCH_MAX_ROTATIONS + k] = MatchPartial{key, n_ties, n_cells};
        }
        __syncthreads(); // (wave_key and wave_ties are free for the next k)
    }
}

__global__ __launch_bounds__(64) void k_match_best(const MatchArgs x)
{
    const int map = (int)blockIdx.x, lane = (int)threadIdx.x, W = x.window;
    const bool has = lane < x.n_rotations;
    const MatchPartial mine = has ? x.partials[(size_t)map * MATCH_MAX_ROTATIONS + lane] : MatchPartial{0ull, 0u, 0u};
    const unsigned long long key = match_wave_max(mine.key);
    const uint32_t ties = match_wave_sum(has && (mine.key >> 32) == (key >> 32) ? mine.ties : 0u);
    const uint32_t cells = (uint32_t)__shfl((int)mine.cells, 0, 64);
    if (lane != 0) return;
    const uint32_t rank = ~(uint32_t)key;
    int32_t *best = x.best + (size_t)map * 6;
    best[0] = (int)((rank >> 14) & 63u);
    best[1] = (int)((rank >> 7) & 127u) - W;
    best[2] = (int)(rank & 127u) - W;
    best[3] = (int)(key >> 32);
    best[4] = (int)cells;
    best[5] = (int)ties;
}

void launch_match(const MatchArgs &x, int n_maps, hipStream_t s)
{
    const int D = 2 * x.window + 1, n_cand = D * D, K = x.n_rotations;
    const int B = std::min(MATCH_MAX_THREADS, (n_cand + 63) / 64 * 64), P = (n_cand + B - 1) / B;
    // as many k per work-group as the totals hold, at most MATCH_GROUP, then evened out over the groups: a function of K and W alone
    const int most = std::max(1, std::min(std::min(K, MATCH_GROUP), MATCH_TOTALS / n_cand));
    const int n_groups = (K + most - 1) / most, group = (K + n_groups - 1) / n_groups;
    const dim3 grid((unsigned)n_maps * (unsigned)n_groups), block((unsigned)B);
    switch (P) {
    case 1: hipLaunchKernelGGL(k_match_scores<1>, grid, block, 0, s, x, group, n_groups); break;
    case 2: hipLaunchKernelGGL(k_match_scores<2>, grid, block, 0, s, x, group, n_groups); break;
    case 3: hipLaunchKernelGGL(k_match_scores<3>, grid, block, 0, s, x, group, n_groups); break;
    case 4: hipLaunchKernelGGL(k_match_scores<4>, grid, block, 0, s, x, group, n_groups); break;
    default: hipLaunchKernelGGL(k_match_scores<MATCH_MAX_PER_THREAD>, grid, block, 0, s, x, group, n_groups); break;
    }
    hipLaunchKernelGGL(k_match_best, dim3((unsigned)n_maps), dim3(64), 0, s, x);
}

} // namespace gg
