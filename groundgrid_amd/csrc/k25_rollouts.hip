// K25 -- gg_score_rollouts: the score of every candidate trajectory ("rollout") of MANY maps in device memory (include/groundgrid_hip.h):
// per rollout the number of leading poses the heading mask admits, what they cost on the cost plane, the least clearance along them and,
// for a rollout that ran to its end, the cost-to-go D of gg_route_headings at its last pose; per map the best rollout.  What a caller
// composes today from K + 2 downloaded planes per map, or in torch from index arithmetic, three gathers, a cumprod and a cumsum over
// [maps, rollouts, steps] tensors.
//
// One launch, one work-group of ROLLOUT_THREADS = 1024 threads per map: no work-group waits for another and d_best needs no second launch.
// Thread `tid` owns rollouts tid, tid + 1024, ... and walks the steps of each in order.  The table is step-major, so the 16-byte entries a
// wavefront loads for one step are 1 KiB of consecutive memory; ROLLOUT_AHEAD = 4 entries are loaded before the first is looked at, because
// an entry's address depends on nothing the walk computes.  Mask, cost and clearance are one gather each per admissible pose, D one gather
// per complete rollout.  Behind the first inadmissible pose only s is looked at (it decides len), and the walk ends at the first s <= 0.
// Every loop carries its bound (P, T).
//
// The table is the caller's device data and is NOT validated: every word has a meaning and none can take an address outside a plane.
//   - the rotated offset is formed in 64 bits: |cq|, |sq| <= 2^14 and |da|, |db| <= 2^31, so |A|, |B| <= 2^46, rha() <= 2^32 and the
//     position r16 + rha(A) < 2^33; the cell is its arithmetic shift by 4, compared with [0, rows) x [0, cols) in 64 bits before
//     anything is addressed.
//   - dk is reduced into [0, K) before k0 is added, so k0 + dk never wraps.
//   - s enters as min(s, 32767); the entry point bounds T * 32767 * cost_max by 2^31 - 2, so `cost` stays inside an int32.
// Integers only; a record is a function of its rollout alone and the best of a map is the minimum of distinct 64-bit keys
// (total << 32 | p), so the result does not depend on the order the atomics arrive in.
#include "gg_device.h"

namespace gg {

constexpr int ROLLOUT_AHEAD = 4; // table entries in flight per rollout
constexpr int32_t ROLLOUT_NONE = GG_ROUTE_NONE;

GG_DEV long long rollout_rha(long long v) { return v < 0 ? -((-v + GG_MATCH_UNIT / 2) >> 14) : (v + GG_MATCH_UNIT / 2) >> 14; }

// Buffers are 4-byte aligned by contract and a stride may be any number of words: the 16-byte forms are taken where the map's row allows it
// (a uniform choice per work-group), four words otherwise
GG_DEV int4 rollout_entry(const int32_t *table, size_t at, bool wide)
{
    if (wide) return reinterpret_cast<const int4 *>(table)[at];
    const int32_t *e = table + 4 * at;
    return make_int4(e[0], e[1], e[2], e[3]);
}
GG_DEV void rollout_store(int32_t *rec, size_t p, bool wide, int4 a, int4 b)
{
    int32_t *w = rec + 8 * p;
    if (wide) {
        reinterpret_cast<int4 *>(w)[0] = a;
        reinterpret_cast<int4 *>(w)[1] = b;
        return;
    }
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
GG_DEV void rollout_best(int32_t *best, int map, int p, int total, int complete, int scored)
{
    int32_t *w = best + 4 * (size_t)map;
    w[0] = p, w[1] = total, w[2] = complete, w[3] = scored;
}

GG_DEV unsigned long long rollout_wave_min(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(ROLLOUT_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_score_rollouts(const RolloutArgs x)
{
    __shared__ unsigned long long best_key;
    __shared__ int n_complete, n_scored;
    const int tid = (int)threadIdx.x, lane = tid & 63, map = (int)blockIdx.x;
    const int P = x.P, T = x.T, K = x.K, rows = x.rows, cols = x.cols;
    if (tid == 0) best_key = ~0ull, n_complete = 0, n_scored = 0;
    __syncthreads();

    const int32_t *st = x.starts + 3 * (size_t)map;
    const int r16 = st[0], c16 = st[1], k0 = st[2]; // (the entry point checked them: inside the map and [0, K), or r16 == -1)
    int32_t *rec = x.records + (size_t)map * x.record_stride;
    const bool wide_rec = (reinterpret_cast<uintptr_t>(rec) & 15u) == 0;
    if (r16 == -1) { // (uniform) no start: nothing is scored
        for (int p = tid; p < P; p += ROLLOUT_THREADS)
            rollout_store(rec, (size_t)p, wide_rec, make_int4(0, 0, 0, -1), make_int4(-1, ROLLOUT_NONE, ROLLOUT_NONE, ROLLOUT_NONE));
        if (x.best && tid == 0) rollout_best(x.best, map, -1, ROLLOUT_NONE, 0, 0);
        return;
    }
    const int row0 = r16 >> 4, col0 = c16 >> 4;
    const long long cq = x.rotations ? x.rotations[k0].x : 0, sq = x.rotations ? x.rotations[k0].y : 0;
    const bool relative = x.frame == GG_ROLLOUTS_RELATIVE, row_major = x.row_major != 0;
    const int32_t *table = x.table + (size_t)map * x.table_stride;
    const bool wide_table = (reinterpret_cast<uintptr_t>(table) & 15u) == 0;
    const uint32_t *mask = x.mask + (size_t)map * x.mask_stride;
    const int32_t *cost = x.cost ? x.cost + (size_t)map * x.cost_stride : nullptr;
    const int32_t *clear = x.clear ? x.clear + (size_t)map * x.clear_stride : nullptr;
    const int32_t *dist = x.dist ? x.dist + (size_t)map * x.dist_stride : nullptr;
    const int start_cell = row_major ? row0 * cols + col0 : col0 * rows + row0;

    unsigned long long my_key = ~0ull;
    int my_complete = 0, my_scored = 0;
    for (int p = tid; p < P; p += ROLLOUT_THREADS) {
        int steps = 0, len = T, sum = 0, min_clear = ROLLOUT_NONE, end_cell = start_cell, end_k = k0;
        bool open = true, walking = true; // open: no inadmissible pose yet; walking: no s <= 0 yet
        for (int t0 = 0; t0 < T && walking; t0 += ROLLOUT_AHEAD) {
            int4 e[ROLLOUT_AHEAD];
#pragma unroll
            for (int j = 0; j < ROLLOUT_AHEAD; ++j) e[j] = rollout_entry(table, (size_t)min(t0 + j, T - 1) * P + p, wide_table);
#pragma unroll
            for (int j = 0; j < ROLLOUT_AHEAD; ++j) {
                if (!walking || t0 + j >= T) break;
                const int da = e[j].x, db = e[j].y, dk = e[j].z, s = e[j].w;
                if (s <= 0) {
                    len = t0 + j;
                    walking = false;
                    break;
                }
                if (!open) continue;
                long long pr = da, pc = db;
                if (relative) {
                    pr = (long long)r16 + rollout_rha(cq * da - sq * db);
                    pc = (long long)c16 + rollout_rha(sq * da + cq * db);
                }
                const long long row = pr >> 4, col = pc >> 4; // (floor)
                bool ok = row >= 0 && row < rows && col >= 0 && col < cols;
                if (ok && x.reach > 0) {
                    const int dr = (int)row - row0, dc = (int)col - col0;
                    ok = dr >= -x.reach && dr <= x.reach && dc >= -x.reach && dc <= x.reach;
                }
                int k = dk % K; // (dk mod K first: k0 + dk itself may not fit an int32)
                k += (k < 0 ? K : 0) + (relative ? k0 : 0);
                k -= k >= K ? K : 0;
                int cell = 0;
                if (ok) {
                    cell = row_major ? (int)row * cols + (int)col : (int)col * rows + (int)row;
                    ok = (mask[cell] >> k) & 1u;
                }
                if (!ok) {
                    open = false;
                    continue;
                }
                const int w = cost ? min(max(cost[cell], 1), x.cost_max) : 1;
                sum += min(s, 32767) * w;
                if (clear) min_clear = min(min_clear, clear[cell]);
                end_cell = cell, end_k = k;
                ++steps;
            }
        }
        const bool complete = steps == len;
        int togo = ROLLOUT_NONE, total = ROLLOUT_NONE;
        if (complete) {
            togo = dist ? dist[(size_t)end_k * x.plane_stride + end_cell] : 0;
            if (togo != ROLLOUT_NONE && togo >= 0) total = (int)min((long long)sum + togo, (long long)ROLLOUT_NONE - 1);
        }
        if (steps == 0) min_clear = ROLLOUT_NONE;
        rollout_store(rec, (size_t)p, wide_rec, make_int4(steps, len, sum, end_cell), make_int4(end_k, togo, min_clear, total));
        my_complete += complete ? 1 : 0;
        if (total != ROLLOUT_NONE) {
            ++my_scored;
            const unsigned long long key = ((unsigned long long)(uint32_t)total << 32) | (uint32_t)p;
            my_key = key < my_key ? key : my_key;
        }
    }
    if (!x.best) return; // (uniform)
    my_key = rollout_wave_min(my_key);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        my_complete += __shfl_xor(my_complete, d, 64);
        my_scored += __shfl_xor(my_scored, d, 64);
    }
    if (lane == 0) {
        if (my_key != ~0ull) atomicMin(&best_key, my_key);
        if (my_complete) atomicAdd(&n_complete, my_complete);
        if (my_scored) atomicAdd(&n_scored, my_scored);
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long key = best_key;
        if (key == ~0ull) rollout_best(x.best, map, -1, ROLLOUT_NONE, n_complete, n_scored);
        else rollout_best(x.best, map, (int)(uint32_t)key, (int)(uint32_t)(key >> 32), n_complete, n_scored);
    }
}

void launch_rollouts(const RolloutArgs &x, int n_maps, hipStream_t s)
{
    hipLaunchKernelGGL(k_score_rollouts, dim3(n_maps), dim3(ROLLOUT_THREADS), 0, s, x);
}

} // namespace gg
