// K23 -- gg_track_clusters: which cluster of the last scan a cluster of this scan is, for MANY maps in device memory
// (include/groundgrid_hip.h): the contingency matrix O[c][p] of this scan's id plane against the shifted id plane of the last scan, gated
// by a (2 g + 1)^2 window; every current cluster's best predecessor p*(c); every predecessor's best claimant; a persistent track id, an age
// and the overlap figures per cluster; fresh ids for the clusters that continue nothing.  What a caller composes today from two downloaded
// planes and a table on the host, or in torch from nonzero, a key c * M + p per offset and a bincount per map.
//
// One launch, one work-group of TRACK_THREADS = 1024 threads per map: everything between the planes and the records lives in the
// work-group's LDS, no work-group waits for another, and every loop carries its bound (cells, clusters, slabs <= ceil(M / 28)).
//   1. walk of the current plane: the largest id (per thread, per wavefront, one LDS max per wavefront) and cells / sum_x / sum_y per
//      cluster by LDS integer adds.  Kc follows.
//   2. the Kc x Kp matrix is held a SLAB at a time: R = slab_words / Kp rows (slab_words = min(M * M, 28 Ki): the whole matrix whenever
//      M <= 168 or Kc * Kp <= 28 Ki, which is the usual hundred clusters).  Per slab: zero it, re-walk the plane -- a cell whose id falls in
//      the slab's rows reads its (2 g + 1)^2 shifted neighbours of the previous plane, consecutive lanes consecutive words of a line, and
//      adds 1 to slab[c - c0][p] per hit -- then one wavefront per row reduces it to the key (O << 32 | ~p), whose maximum is the largest
//      O and among equals the smallest p, and lane 0 offers (O << 32 | ~c) to the predecessor's word with one 64-bit LDS max: the winner.
//   3. thread c decides inheritance (the winner's word of p*(c) names c), the new clusters are ranked by ballot and popcount within a
//      wavefront and a sum over the sixteen wavefront counts, and the track ids go to LDS.
//   4. last walk: `still` (the cell's own shifted word equals the predecessor) by LDS adds, and the d_cell_track plane when it is asked
//      for, a coalesced store per cell.  Skipped when there is neither.
//   5. thread c writes record c; thread 0 the four head words.  Records from Kc on and words beyond rows * cols are never addressed.
// Integers only: adds commute and the keys of a maximum differ (by p within a row, by c within a column), so the result does not depend on
// the order the atomics arrive in.  The entry point bounds rows * cols * max(rows, cols) by 2^31 - 1: sum_x, sum_y and O (<= 81 cells)
// stay inside an int32.  The shift arrives clamped to [-nx, nx] x [-ny, ny], so x + sx + a stays inside an int32; from |s| = side on the
// definition says nothing overlaps whatever the gate, which is one uniform test here.
//
// LDS: 9 words per cluster of M (winner keys 2, cells, sum_x, sum_y, p*, O, still, track id) + 64 + the slab: 18.5 KiB at M = 64 and
// 68.8 KiB at M = 128 (the slab is M * M), 121.3 KiB at M = 256, 148.3 KiB at M = 1024 -- one work-group of sixteen wavefronts per compute
// unit from M = 139 on (two no longer fit 160 KiB).
#include "gg_device.h"

namespace gg {

constexpr int TRACK_WAVES = TRACK_THREADS / 64;
constexpr uint32_t TRACK_NOT = 0xFFFFFFFFu;

GG_DEV unsigned long long track_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// One walk of a map's id plane: f(i, id) for every cell i, thread `tid` taking cells tid, tid + TRACK_THREADS, ...  Four loads are issued
// before the first use -- most cells hold -1 and cost nothing but their load, so the walk is as fast as its loads are deep.
template <class F> GG_DEV void track_walk(const int32_t *cur, int C, int tid, F f)
{
    int i = tid;
    for (; i + 3 * TRACK_THREADS < C; i += 4 * TRACK_THREADS) {
        const int a = cur[i], b = cur[i + TRACK_THREADS], c = cur[i + 2 * TRACK_THREADS], d = cur[i + 3 * TRACK_THREADS];
        f(i, a);
        f(i + TRACK_THREADS, b);
        f(i + 2 * TRACK_THREADS, c);
        f(i + 3 * TRACK_THREADS, d);
    }
    for (; i < C; i += TRACK_THREADS) f(i, cur[i]);
}

__global__ __launch_bounds__(TRACK_THREADS) void k_track_clusters(const TrackArgs x)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t track_smem[];
    const int M = x.M, nx = x.nx, ny = x.ny, C = nx * ny, g = x.gate;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, map = (int)blockIdx.x;
    unsigned long long *win = reinterpret_cast<unsigned long long *>(track_smem); // [M] per predecessor: (O << 32 | ~c) of its best claimant
    int32_t *cnt = reinterpret_cast<int32_t *>(track_smem + 2 * (size_t)M);       // [M] each, per current cluster:
    int32_t *sum_x = cnt + M, *sum_y = sum_x + M;
    int32_t *pstar = sum_y + M;   // p*(c), -1: none; from step 3 on -1 unless c inherits
    int32_t *ov = pstar + M;      // O[c][p*(c)]
    int32_t *still = ov + M;
    int32_t *track = still + M;   // the track id
    int32_t *misc = track + M;    // [TRACK_MISC_WORDS]: 0 the largest id; 8 + w / 24 + w: new / inheriting clusters of wavefront w
    uint32_t *slab = reinterpret_cast<uint32_t *>(misc + TRACK_MISC_WORDS);

    const int32_t *cur = x.cells + (size_t)map * x.cells_stride;
    const int32_t *prv = x.prev ? x.prev + (size_t)map * x.prev_stride : nullptr;
    const gg_track *tin = x.prev ? x.tracks_in + (size_t)map * M : nullptr;

    for (int c = tid; c < M; c += TRACK_THREADS) {
        win[c] = 0ull;
        cnt[c] = sum_x[c] = sum_y[c] = ov[c] = still[c] = 0;
        pstar[c] = track[c] = -1;
    }
    if (tid == 0) misc[0] = -1;
    __syncthreads();

    // 1. the largest id, and the cells and coordinate sums of every cluster
    int top = -1;
    track_walk(cur, C, tid, [&](int i, int id) {
        top = max(top, id);
        if (id >= 0 && id < M) {
            const int y = i / nx, xx = i - y * nx;
            atomicAdd(&cnt[id], 1);
            atomicAdd(&sum_x[id], xx);
            atomicAdd(&sum_y[id], y);
        }
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) top = max(top, __shfl_xor(top, d, 64));
    if (lane == 0 && top >= 0) atomicMax(&misc[0], top);
    __syncthreads();
    const int Kc = misc[0] >= M - 1 ? M : misc[0] + 1;
    const int Kp = prv ? min(max(x.heads_in[(size_t)map * 4 + 1], 0), M) : 0;
    const uint32_t next_id = prv ? (uint32_t)x.heads_in[(size_t)map * 4 + 0] : 0u;
    const int2 sh = x.shifts ? x.shifts[map] : make_int2(0, 0);
    const bool meets = Kc > 0 && Kp > 0 && sh.x > -nx && sh.x < nx && sh.y > -ny && sh.y < ny; // (uniform)

    // 2. the contingency matrix, a slab of rows at a time
    if (meets) {
        const int R = x.slab_words / Kp; // >= 1: slab_words >= min(M * M, 1024) >= Kp
        for (int c0 = 0; c0 < Kc; c0 += R) {
            const int rows = min(R, Kc - c0);
            for (int i = tid; i < rows * Kp; i += TRACK_THREADS) slab[i] = 0u;
            __syncthreads();
            track_walk(cur, C, tid, [&](int i, int id) {
                if (id < c0 || id >= c0 + rows) return;
                const int y = i / nx, xx = i - y * nx;
                uint32_t *row = slab + (size_t)(id - c0) * Kp;
                for (int b = -g; b <= g; ++b) {
                    const int py = y + sh.y + b;
                    if (py < 0 || py >= ny) continue;
                    for (int a = -g; a <= g; ++a) {
                        const int px = xx + sh.x + a;
                        if (px < 0 || px >= nx) continue;
                        const int p = prv[py * nx + px];
                        if (p >= 0 && p < Kp) atomicAdd(&row[p], 1u);
                    }
                }
            });
            __syncthreads();
            for (int r = wave; r < rows; r += TRACK_WAVES) { // (uniform per wavefront)
                const uint32_t *row = slab + (size_t)r * Kp;
                unsigned long long key = 0ull;
                for (int p = lane; p < Kp; p += 64) {
                    const uint32_t o = row[p];
                    const unsigned long long k = o ? ((unsigned long long)o << 32) | (TRACK_NOT - (uint32_t)p) : 0ull;
                    key = k > key ? k : key;
                }
                key = track_wave_max(key);
                if (lane == 0 && key) {
                    const int c = c0 + r, p = (int)(TRACK_NOT - (uint32_t)key);
                    pstar[c] = p;
                    ov[c] = (int32_t)(key >> 32);
                    atomicMax(&win[p], (key & 0xFFFFFFFF00000000ull) | (TRACK_NOT - (uint32_t)c));
                }
            }
            __syncthreads();
        }
    }

    // 3. inheritance, the rank of the new clusters, the track ids (thread c speaks for cluster c: TRACK_THREADS >= M)
    const int c = tid;
    const bool valid = c < Kc;
    int p = -1;
    if (valid && pstar[c] >= 0 && (uint32_t)win[pstar[c]] == TRACK_NOT - (uint32_t)c) p = pstar[c];
    const bool inherits = p >= 0, born = valid && !inherits;
    const unsigned long long born_mask = __ballot(born), kept_mask = __ballot(inherits);
    if (lane == 0) {
        misc[8 + wave] = __popcll(born_mask);
        misc[24 + wave] = __popcll(kept_mask);
    }
    if (valid && !inherits) pstar[c] = -1; // (only thread c reads or writes pstar[c] here)
    __syncthreads();
    int before = 0, n_born = 0, n_kept = 0;
#pragma unroll
    for (int w = 0; w < TRACK_WAVES; ++w) {
        before += w < wave ? misc[8 + w] : 0;
        n_born += misc[8 + w];
        n_kept += misc[24 + w];
    }
    int32_t id_out = -1, age = 0;
    if (inherits) {
        id_out = tin[p].track_id;
        age = min(tin[p].age, INT32_MAX - 1) + 1;
    } else if (born) {
        id_out = (int32_t)((next_id + (uint32_t)(before + rank_below(born_mask))) & 0x7FFFFFFFu);
    }
    if (valid) track[c] = id_out;
    __syncthreads();

    // 4. `still` of the inheriting clusters and the d_cell_track plane
    int32_t *cell_track = x.cell_track ? x.cell_track + (size_t)map * x.track_stride : nullptr;
    if (cell_track || (meets && n_kept > 0)) { // (uniform)
        track_walk(cur, C, tid, [&](int i, int id) {
            const bool in = id >= 0 && id < M;
            if (in && meets && pstar[id] >= 0) {
                const int y = i / nx, xx = i - y * nx, px = xx + sh.x, py = y + sh.y;
                if (px >= 0 && px < nx && py >= 0 && py < ny && prv[py * nx + px] == pstar[id]) atomicAdd(&still[id], 1);
            }
            if (cell_track) cell_track[i] = in ? track[id] : -1;
        });
        __syncthreads();
    }

    // 5. the records and the head
    if (valid) {
        gg_track t;
        t.track_id = id_out;
        t.age = age;
        t.prev = p;
        t.overlap = inherits ? ov[c] : 0;
        t.still = inherits ? still[c] : 0;
        t.cells = cnt[c];
        t.sum_row = x.row_major ? sum_y[c] : sum_x[c];
        t.sum_col = x.row_major ? sum_x[c] : sum_y[c];
        x.tracks_out[(size_t)map * M + c] = t;
    }
    if (tid == 0) {
        int32_t *h = x.heads_out + (size_t)map * 4;
        h[0] = (int32_t)((next_id + (uint32_t)n_born) & 0x7FFFFFFFu);
        h[1] = Kc;
        h[2] = n_born;
        h[3] = Kp - n_kept;
    }
}

void launch_tracks(const TrackArgs &x, int n_maps, hipStream_t s)
{
    const size_t lds = track_lds_bytes(x.M, x.slab_words);
    static PerDeviceOnce big_lds;
    if (lds > 64 * 1024)
        big_lds.run([] { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_track_clusters), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024); });
    hipLaunchKernelGGL(k_track_clusters, dim3(n_maps), dim3(TRACK_THREADS), lds, s, x);
}

} // namespace gg
