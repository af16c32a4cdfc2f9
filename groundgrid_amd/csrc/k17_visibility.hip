// K17 -- gg_visibility_clouds: FREE, UNKNOWN and OCCUPIED cells of MANY labelled clouds in device memory (include/groundgrid_hip.h): the
// occupancy of gg_cluster_clouds, and FREE where a return landed or the integer ray from the sensor cell to the cell of a return passed.
// What a caller composes today from a download of the clouds and a ray walk per point on the host.
//
// The d_state plane is the only global working memory (one 32-bit word per cell).  After launch_cluster_occupancy (k15_cluster.hip: the
// same three launches on the same kind of plane) a word is the cell's index L (occupied, < 2^30) or 0xFFFFFFFF; from there on the two bits
// below the sign of a word that is NOT occupied are flags that are only ever CLEARED: bit 30 = "no return landed here", bit 29 = "no ray
// crossed here".  An occupied word is never written again: it has both bits clear, as it should (a participating point is a return).
//   k_visibility_hits    the walk of cloud_walk.h over the points of label 49 / 99: word[cell] := 0xBFFFFFFF where it is 0xFFFFFFFF -- every
//                        writer stores the same word
//   k_visibility_trace   S work-groups per cloud ("shares"), each with a bitmap of the map in LDS, one bit per cell, zeroed.  A share takes
//                        every S-th 64-cell window of the plane per wavefront; the cells of a window whose bit 30 is clear are END CELLS,
//                        and the wavefront walks them one by one, its lanes along the ray: step k of the closed form is independent of
//                        every other, so lane l takes k = l, l + 64, ...; a step sets its bit in LDS (read first: 93 % of the steps of a
//                        64-ring scan find it set, and a same-address LDS atomic runs one lane at a time).  Then the share clears bit 29
//                        of the words of its set bits (one global atomicAnd per CROSSED CELL that still has the bit, none per ray step).
//                        The set of end cells is bit 30 of the global words, fixed by the launch before; crossed cells go to LDS and to
//                        bit 29 -- no share can take a crossed cell for an end cell, whatever the order in which shares finish (the ray
//                        to a crossed cell is in general no prefix of the ray that crossed it).
//   k_visibility_states  word >= 0 as an int32: OCCUPIED; 0xFFFFFFFF: UNKNOWN; else FREE.  The three counts are added up per work-group of
//                        2048 cells, which sends at most one integer atomic add per state.
// There is ONE path for every geometry and every number of clouds: the bitmap of the largest map (1000 x 1000: 125 000 bytes) fits the
// 160 KiB of a CU beside nothing else, so nothing else is kept there; a map whose bitmap would not fit is refused by the entry point
// (VISIBILITY_MAX_CELLS).  The number of shares only changes which work-group walks which window.
// The minor coordinate of step k is q = (2 k m + n) / (2 n) with m = min(|dr|, |dc|) <= n = max(|dr|, |dc|) (the major one is k itself:
// (2 k n + n) / (2 n) = k).  2 k m + n < 2 n n + n < 2^24 for n <= 1143, so numerator and denominator are exact floats, the float quotient
// is within one of q, and two integer comparisons make it q: no integer division per step.
// No work-group waits for another, every loop is bounded by rows * cols, no float decides anything and only integer atomics (add, and,
// LDS or) are used: the outputs do not depend on scheduling.
//
// Algorithmic bytes: the occupancy as K15's; the hits per input point 1 (labels; 0.25 with masks) + 16 (32: GG_POINT32) and per return in
// the map 4 read (+ 4 written once per hit cell); the trace per cell 4 read, per crossed cell 4 read + one 4-byte atomic; the states per
// cell 4 read + 4 written.  Operations: per ray step a dozen integer and float operations, an LDS read and, for a bit not yet set, an LDS
// atomic (674 M steps per 1024 headline clouds).
#include <algorithm>

#include "cloud_walk.h"

namespace gg {

constexpr uint32_t VIS_EMPTY = 0xFFFFFFFFu;   // not occupied, no return, not crossed (launch_cluster_occupancy's word)
constexpr uint32_t VIS_NO_HIT = 0x40000000u;  // bit 30 of a word that is not occupied: no return landed in the cell
constexpr uint32_t VIS_NO_RAY = 0x20000000u;  // bit 29 ...: no ray crossed the cell
constexpr int VIS_THREADS = 1024;             // of a share: 16 wavefronts
constexpr int VIS_MAX_SHARES = 32;
constexpr int VIS_STATE_CELLS = 2048;         // cells per work-group of k_visibility_states

GG_DEV uint32_t visibility_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (cloud, item) of a work-group, grid (items, clouds): a cloud's work-groups meet in one L2
GG_DEV void visibility_item(int &cloud, int &item)
{
    const uint32_t it = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    cloud = (int)(it / gridDim.x);
    item = (int)(it % gridDim.x);
}

template <int FMT, bool MASKS>
__global__ __launch_bounds__(256) void k_visibility_hits(const Arena a, const VisibilityArgs x)
{
    CloudChunk k;
    if (!cloud_chunk(a, x.occ.cl, k) || k.base >= k.end) return; // (uniform over the wavefront; there is no barrier below)
    uint32_t *plane = x.state + (size_t)k.io * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    CloudFrame f;
    load_cloud_frame(a, x.occ.cl.clouds[k.cloud], f);
    walk_chunk<FMT, MASKS, WALK_POINT>(x.occ.cl, k, [&](int, uint32_t sel, const uint4 &v, uint32_t) GG_INLINE_LAMBDA {
        if (sel == 0u) return; // (no cross-lane operation in this body)
        float px = __uint_as_float(v.x), py = __uint_as_float(v.y), pz = __uint_as_float(v.z);
        int r, cc;
        if (!locate_point(a, f, px, py, pz, r, cc)) return;
        uint32_t *w = plane + linear_cell(a, row_major, r, cc);
        if (visibility_load(w) == VIS_EMPTY) *w = VIS_EMPTY & ~VIS_NO_HIT; // (an occupied word stays; every writer stores this word)
    });
}

// floor(num / den) for 0 <= num < 2^24, 0 < den < 2^24, inv_den = 1 / den to a few ulp: both are exact as floats and the quotient is below
// 2^11, so the float product is within one of the integer quotient
GG_DEV int visibility_quotient(int num, int den, float inv_den)
{
    int q = (int)((float)num * inv_den);
    if (q * den > num) --q;
    else if ((q + 1) * den <= num) ++q;
    return q;
}

// Grid (shares, clouds), VIS_THREADS threads, x.bitmap_words words of dynamic LDS.
__global__ __launch_bounds__(VIS_THREADS) void k_visibility_trace(const Arena a, const VisibilityArgs x)
{
    extern __shared__ uint32_t crossed[];
    int cloud, share;
    visibility_item(cloud, share);
    const SplitCloud &cl = x.occ.cl.clouds[cloud];
    CloudFrame f;
    load_cloud_frame(a, cl, f);
    int r0, c0;
    if (!cell_of_point(a, f, cl.ox, cl.oy, r0, c0)) return; // the sensor is in no cell: no ray (uniform over the work-group)
    const int C = a.g.C, rows = a.g.rows, cols = a.g.cols;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const int minors = row_major ? cols : rows;
    uint32_t *plane = x.state + (size_t)cl.io_index * x.plane_stride;
    for (int i = (int)threadIdx.x; i < x.bitmap_words; i += VIS_THREADS) crossed[i] = 0u;
    __syncthreads();
    const int waves = VIS_THREADS / 64, wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int windows = (C + 63) / 64;
    for (int w = share * waves + wave; w < windows; w += (int)gridDim.x * waves) { // (uniform over the wavefront)
        const int L = w * 64 + lane;
        const int major = L / minors, minor = L - major * minors; // (one division per window: a ray reads its end cell from its lane)
        const int my_r = row_major ? major : minor, my_c = row_major ? minor : major;
        unsigned long long ends = __ballot(L < C && (visibility_load(plane + L) & VIS_NO_HIT) == 0u);
        while (ends) {
            const int src = __ffsll((long long)ends) - 1; // (uniform: `ends` is)
            ends &= ends - 1ull;
            const int dr = __builtin_amdgcn_readlane(my_r, src) - r0, dc = __builtin_amdgcn_readlane(my_c, src) - c0;
            const int ar = abs(dr), ac = abs(dc), sgr = dr < 0 ? -1 : 1, sgc = dc < 0 ? -1 : 1;
            const int n = max(ar, ac), m = min(ar, ac);
            const int steps = x.max_cells > 0 ? min(n, x.max_cells) : n; // (n == 0: nothing)
            const float inv = __builtin_amdgcn_rcpf((float)(2 * n)); // (one ulp: visibility_quotient corrects by one either way)
            for (int k = lane; k < steps; k += 64) {
                const int q = visibility_quotient(2 * k * m + n, 2 * n, inv);
                const int cell = linear_cell(a, row_major, r0 + sgr * (ar >= ac ? k : q), c0 + sgc * (ar >= ac ? q : k));
                const uint32_t bit = 1u << (cell & 31);
                uint32_t *word = crossed + (cell >> 5);
                if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit) == 0u) atomicOr(word, bit);
            }
        }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < x.bitmap_words; i += VIS_THREADS) {
        uint32_t bits = crossed[i];
        while (bits) {
            uint32_t *w = plane + i * 32 + __ffs((int)bits) - 1; // (< C: only cells of the map were set)
            bits &= bits - 1u;
            const uint32_t v = visibility_load(w);
            if ((v >> 31) && (v & VIS_NO_RAY)) atomicAnd(w, ~VIS_NO_RAY); // (not occupied, and nobody cleared it yet)
        }
    }
}

// Grid (ceil(C / VIS_STATE_CELLS), clouds), 256 threads, VIS_STATE_CELLS / 256 cells per thread, 256 apart.  A work-group adds its
// counts up (lanes, then its four wavefronts through LDS) and sends at most three atomics: per wavefront they cost more than the rest
// of the call (measured: 4.6 against 0.35 ms per 1024 headline maps).
__global__ __launch_bounds__(256) void k_visibility_states(const Arena a, const VisibilityArgs x)
{
    __shared__ uint32_t wave_counts[4][2];
    int cloud, chunk;
    visibility_item(cloud, chunk);
    const int io = x.occ.cl.clouds[cloud].io_index;
    uint32_t *plane = x.state + (size_t)io * x.plane_stride;
    const int first = chunk * VIS_STATE_CELLS, end = min(first + VIS_STATE_CELLS, a.g.C);
    uint32_t n_free = 0u, n_occupied = 0u;
#pragma unroll
    for (int j = 0; j < VIS_STATE_CELLS / 256; ++j) {
        const int L = first + j * 256 + (int)threadIdx.x;
        if (L < end) {
            const uint32_t v = plane[L];
            const int state = (v >> 31) == 0u ? GG_CELL_OCCUPIED : v == VIS_EMPTY ? GG_CELL_UNKNOWN : GG_CELL_FREE;
            plane[L] = (uint32_t)state;
            n_free += state == GG_CELL_FREE;
            n_occupied += state == GG_CELL_OCCUPIED;
        }
    }
    if (!x.counts) return; // (uniform)
    n_free = wave_sum(n_free); // (all 64 lanes are here)
    n_occupied = wave_sum(n_occupied);
    if ((threadIdx.x & 63) == 0) {
        wave_counts[threadIdx.x >> 6][0] = n_free;
        wave_counts[threadIdx.x >> 6][1] = n_occupied;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n_f = (int)(wave_counts[0][0] + wave_counts[1][0] + wave_counts[2][0] + wave_counts[3][0]);
    const int n_o = (int)(wave_counts[0][1] + wave_counts[1][1] + wave_counts[2][1] + wave_counts[3][1]);
    int32_t *counts = x.counts + (size_t)io * 3; // free, unknown, occupied
    if (n_f) atomicAdd(counts + 0, n_f);
    if (end - first - n_f - n_o) atomicAdd(counts + 1, end - first - n_f - n_o);
    if (n_o) atomicAdd(counts + 2, n_o);
}

void launch_visibility(const Arena &a, const VisibilityArgs &x, int n_clouds, hipStream_t s)
{
    launch_cluster_occupancy(a, x.occ, n_clouds, s);
    const dim3 chunks((x.occ.cl.nch + 3) / 4, n_clouds);
    dispatch_cloud_variant(x.occ.cl, [&](auto fmt, auto masks) {
        hipLaunchKernelGGL((k_visibility_hits<decltype(fmt)::value, decltype(masks)::value>), chunks, dim3(256), 0, s, a, x);
    });
    const size_t lds = sizeof(uint32_t) * (size_t)x.bitmap_words; // (<= VISIBILITY_LDS_MAX: the entry point refuses a larger map)
    static PerDeviceOnce big_lds;
    if (lds > 64 * 1024)
        big_lds.run([] { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_visibility_trace), hipFuncAttributeMaxDynamicSharedMemorySize, (int)VISIBILITY_LDS_MAX); });
    // shares per cloud: about two work-groups per CU in a launch of few clouds, one share per cloud from 512 clouds on; never more than
    // there are 64-cell windows for its wavefronts
    const int windows = (a.g.C + 63) / 64;
    const int shares = std::max(1, std::min({VIS_MAX_SHARES, 512 / n_clouds, (windows + VIS_THREADS / 64 - 1) / (VIS_THREADS / 64)}));
    hipLaunchKernelGGL(k_visibility_trace, dim3(shares, n_clouds), dim3(VIS_THREADS), lds, s, a, x);
    if (x.counts) (void)hipMemsetAsync(x.counts, 0, sizeof(int32_t) * 3 * (size_t)n_clouds, s);
    hipLaunchKernelGGL(k_visibility_states, dim3((a.g.C + VIS_STATE_CELLS - 1) / VIS_STATE_CELLS, n_clouds), dim3(256), 0, s, a, x);
}

} // namespace gg
