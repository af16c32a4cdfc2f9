// K24 -- gg_box_clusters: the oriented box of every obstacle cluster of MANY clouds in device memory (include/groundgrid_hip.h): per
// cluster and per candidate heading the extent of the cluster's points along and across the heading, the heading of the smallest integer
// cost (the rectangle's area, or the sum of the points' distances to their nearest edge), one 32-byte record per cluster and optionally
// the whole cost volume.  What a caller composes today from the downloaded ids and points, or in torch from one scatter_reduce per heading
// and per map.
//
// One launch, one work-group of BOX_THREADS = 1024 threads per cloud: everything between the points and the records lives in the
// work-group's LDS, the barrier between "extrema final" and "edge sums" is a __syncthreads, no work-group waits for another, and every
// loop carries its bound (points, headings <= 32, slabs <= ceil(M_i / S)).
//   0. S = box_slab_clusters(K, M) clusters lie in LDS at a time, per (cluster, heading) four int32 extrema and one 64-bit sum, per
//      cluster a point count.  A cloud with M_i <= S is one slab; otherwise the ids are re-walked once per slab.
//   1. walk of the ids, 4 bytes per point, coalesced, four loads in flight; a point's 16 bytes are loaded only when its id falls into
//      the slab (the four loads of a thread again before the first use).  to_map_frame and cell_of_point (cloud_walk.h) decide
//      participation, one subtraction and one multiplication in double quantise, and per heading the two projections meet the extrema:
//      the current extremum is READ first and the LDS atomic issued only when the point improves it -- after the first few points of a
//      cluster almost none do.
//   2. GG_BOX_EDGE only: the same walk again, min(a - a_min, a_max - a, b - b_min, b_max - b) added to the pair's 64-bit sum by one LDS
//      add per (point, heading); a point on an edge adds nothing and issues nothing.  GG_BOX_AREA needs no second walk.
//   3. the cost rows go out coalesced (consecutive threads, consecutive words of the slab's part of d_costs); thread r picks k* of
//      cluster c0 + r by a strict < in ascending k -- the smallest k among equals -- and writes the record.
// Integers only behind the quantisation: minima, maxima and adds commute, so the result does not depend on the order the atomics arrive
// in.  The entry point bounds the side by 4096 cells: |u| <= 32769, and |a|, |b| <= 32769 * 32768 < 2^31.
#include "cloud_walk.h"

namespace gg {

// One walk of a cloud's ids: body(r, v) for every point whose id lies in [c0, c0 + rows), r = id - c0 and v the point's first 16 bytes.
// Thread `tid` takes points tid, tid + BOX_THREADS, ...; (uint32_t)id - c0 < rows is the one test that refuses every id outside the slab,
// -1 and INT32_MIN included.
template <class Body> GG_DEV void box_walk(const int32_t *ids, const uint4 *pts, int mul, int n, int tid, uint32_t c0, uint32_t rows, Body body)
{
    constexpr int ITEMS = 4;
    for (int p0 = tid; p0 < n; p0 += ITEMS * BOX_THREADS) {
        uint32_t r[ITEMS];
        uint4 v[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int p = p0 + j * BOX_THREADS;
            r[j] = p < n ? (uint32_t)ids[p] - c0 : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            if (r[j] < rows) v[j] = pts[(size_t)(p0 + j * BOX_THREADS) * mul];
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j)
            if (r[j] < rows) body(r[j], v[j]);
    }
}

// participation and quantisation of one point: false when it lies in no cell of its map
GG_DEV bool box_units(const Arena &a, const CloudFrame &f, double scale, const uint4 &v, int &ux, int &uy)
{
    float px = __uint_as_float(v.x), py = __uint_as_float(v.y), pz = __uint_as_float(v.z);
    int r, cc;
    if (!locate_point(a, f, px, py, pz, r, cc)) return false;
    ux = (int)floor(((double)px - f.pos_x) * scale); // (inside the map: |.| <= 8 * side + 1)
    uy = (int)floor(((double)py - f.pos_y) * scale);
    return true;
}

__global__ __launch_bounds__(BOX_THREADS) void k_box_clusters(const Arena a, const BoxArgs x)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long box_smem[];
    const int tid = (int)threadIdx.x, K = x.K, S = x.slab;
    unsigned long long *sum = box_smem;                         // [S][K] the edge sums
    int32_t *a_min = reinterpret_cast<int32_t *>(sum + (size_t)S * K); // [S][K] each
    int32_t *a_max = a_min + (size_t)S * K, *b_min = a_max + (size_t)S * K, *b_max = b_min + (size_t)S * K;
    int32_t *cnt = b_max + (size_t)S * K;                       // [S] participating points
    int32_t *rot = cnt + S;                                     // [K][2]

    const SplitCloud &c = x.cl.clouds[blockIdx.x];
    const int n = c.n_points, io = c.io_index;
    CloudFrame f;
    load_cloud_frame(a, c, f);
    const int32_t *ids = x.point_cluster + (size_t)io * x.cl.cloud_stride;
    const int mul = x.cl.point_format == GG_POINT16 ? 1 : 2;
    const uint4 *pts = reinterpret_cast<const uint4 *>(x.cl.points) + (size_t)io * x.cl.cloud_stride * mul;
    const int Mi = min(max(x.n_clusters[io], 0), x.M);
    gg_box *boxes = x.boxes + (size_t)io * x.M;
    unsigned long long *costs = x.costs ? x.costs + (size_t)io * x.M * K : nullptr;
    const bool edge = x.criterion == GG_BOX_EDGE;
    const double scale = x.scale;
    if (tid < 2 * K) rot[tid] = x.rot[tid];

    for (int c0 = 0; c0 < Mi; c0 += S) {
        const int rows = min(S, Mi - c0), pairs = rows * K;
        for (int i = tid; i < pairs; i += BOX_THREADS) {
            sum[i] = 0ull;
            a_min[i] = b_min[i] = INT32_MAX;
            a_max[i] = b_max[i] = INT32_MIN;
        }
        for (int i = tid; i < rows; i += BOX_THREADS) cnt[i] = 0;
        __syncthreads();

        // 1. the extrema and the point counts
        box_walk(ids, pts, mul, n, tid, (uint32_t)c0, (uint32_t)rows, [&](uint32_t r, const uint4 &v) GG_INLINE_LAMBDA {
            int ux, uy;
            if (!box_units(a, f, scale, v, ux, uy)) return;
            atomicAdd(&cnt[r], 1);
            const int at = (int)r * K;
            for (int k = 0; k < K; ++k) {
                const int cq = rot[2 * k], sq = rot[2 * k + 1];
                const int pa = ux * cq + uy * sq, pb = uy * cq - ux * sq;
                // (plain reads beside other lanes' atomics: an extremum only ever improves, so a stale word is a WORSE extremum and costs at
                // most an atomic that changes nothing; a point that improves the true extremum also improves the stale one and is never skipped)
                if (pa < a_min[at + k]) atomicMin(&a_min[at + k], pa);
                if (pa > a_max[at + k]) atomicMax(&a_max[at + k], pa);
                if (pb < b_min[at + k]) atomicMin(&b_min[at + k], pb);
                if (pb > b_max[at + k]) atomicMax(&b_max[at + k], pb);
            }
        });
        __syncthreads();

        // 2. the edge sums, against the final extrema
        if (edge) { // (uniform)
            box_walk(ids, pts, mul, n, tid, (uint32_t)c0, (uint32_t)rows, [&](uint32_t r, const uint4 &v) GG_INLINE_LAMBDA {
                int ux, uy;
                if (!box_units(a, f, scale, v, ux, uy)) return;
                const int at = (int)r * K;
                for (int k = 0; k < K; ++k) {
                    const int cq = rot[2 * k], sq = rot[2 * k + 1];
                    const uint32_t pa = (uint32_t)(ux * cq + uy * sq), pb = (uint32_t)(uy * cq - ux * sq);
                    // (each difference is >= 0 and < 2^32: the unsigned subtraction is exact)
                    const uint32_t da = min(pa - (uint32_t)a_min[at + k], (uint32_t)a_max[at + k] - pa);
                    const uint32_t db = min(pb - (uint32_t)b_min[at + k], (uint32_t)b_max[at + k] - pb);
                    const uint32_t d = min(da, db);
                    if (d) atomicAdd(&sum[at + k], (unsigned long long)d);
                }
            });
            __syncthreads();
        }

        // 3. the cost rows, k* and the records
        const auto cost_of = [&](int r, int i) -> unsigned long long {
            if (cnt[r] == 0) return ~0ull;
            if (edge) return sum[i];
            return (unsigned long long)((long long)a_max[i] - (long long)a_min[i]) * (unsigned long long)((long long)b_max[i] - (long long)b_min[i]);
        };
        if (costs)
            for (int i = tid; i < pairs; i += BOX_THREADS) costs[(size_t)c0 * K + i] = cost_of(i / K, i);
        for (int r = tid; r < rows; r += BOX_THREADS) {
            gg_box t;
            t.heading = -1;
            t.points = t.a_min = t.a_max = t.b_min = t.b_max = t.cost_lo = t.cost_hi = 0;
            if (cnt[r] > 0) {
                int best = 0;
                unsigned long long least = cost_of(r, r * K);
                for (int k = 1; k < K; ++k) {
                    const unsigned long long v = cost_of(r, r * K + k);
                    if (v < least) least = v, best = k;
                }
                const int i = r * K + best;
                t.heading = best;
                t.points = cnt[r];
                t.a_min = a_min[i];
                t.a_max = a_max[i];
                t.b_min = b_min[i];
                t.b_max = b_max[i];
                t.cost_lo = (int32_t)(uint32_t)least;
                t.cost_hi = (int32_t)(uint32_t)(least >> 32);
            }
            boxes[c0 + r] = t;
        }
        __syncthreads(); // (the next slab re-initialises what this one still reads)
    }
}

void launch_boxes(const Arena &a, const BoxArgs &x, int n_clouds, hipStream_t s)
{
    const size_t lds = box_lds_bytes(x.K, x.slab);
    static PerDeviceOnce big_lds;
    if (lds > 64 * 1024)
        big_lds.run([] { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_box_clusters), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024); });
    hipLaunchKernelGGL(k_box_clusters, dim3(n_clouds), dim3(BOX_THREADS), lds, s, a, x);
}

} // namespace gg
