// K12 -- gg_split_clouds: the ground and the non-ground points of MANY labelled clouds as dense clouds in device memory, with every point's
// height above the estimated terrain and its index in the input cloud (include/groundgrid_hip.h).  What a consumer behind the segmenter
// gets today with `points[labels == 99]` per cloud -- a launch and a device -> host synchronisation per cloud, the output size being data
// dependent -- in two launches for the whole batch and with the counts left on the device.
//
// Both launches use the wave <-> chunk mapping of K1 / K5 / K8 (a.PW points per wavefront, four wavefronts per work-group, grid
// (ceil(nch / 4), clouds), xcd_contiguous_item: the chunks of a cloud share an L2):
//   k_split_count     the number of 49s and of 99s among the labels of every (cloud, chunk) -> one pair in call scratch.  Ballots and
//                     popcounts: no atomics, nothing depends on an arrival order.
//   k_split_scatter   a wavefront sums the pairs of its cloud's EARLIER chunks (at most max_points / PW of them: a strided read and a wave
//                     reduction) -- its first free element in either set, so no third launch scans them and no work-group ever waits
//                     for another --, work-group 0 of a cloud writes the two totals, and the chunk is walked in 64-point windows, four
//                     windows' loads in flight as in k_score: a selected point's rank inside the window is a ballot and rank_below, its
//                     record one 16-byte store, height and source 4-byte stores.  The ground under a point is gathered only where a
//                     height is asked for and the point lies inside the map.
// Order inside a set is the cloud's own (ascending point index): windows, chunks and lanes are all ranked in that order.
//
// Algorithmic bytes per input point: 1 (labels; 0.25 with masks) in the count, 1 + 16 (32: GG_POINT32) in the scatter, plus per selected
// point 8 gathered (the (ground, confidence) pair) and 16 + 4 + 4 written.
#include "gg_device.h"

namespace gg {

template <bool MASKS> GG_DEV const uint8_t *split_label_row(const SplitArgs &x, int io)
{
    return MASKS ? x.masks + (size_t)io * ((x.cloud_stride + 3) / 4) : x.labels + (size_t)io * x.cloud_stride;
}

GG_DEV uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

template <bool MASKS>
__global__ __launch_bounds__(256) void k_split_count(const Arena a, const SplitArgs x)
{
    const uint32_t item = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int cloud = (int)(item / gridDim.x), bx = (int)(item % gridDim.x);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = bx * 4 + wave;
    if (chunk >= x.nch) return; // (uniform over the wavefront)
    const int n = x.clouds[cloud].n_points, io = x.clouds[cloud].io_index;
    const int base = min(chunk * a.PW, n);
    const int end = min(base + a.PW, n);
    const uint8_t *row = split_label_row<MASKS>(x, io);

    uint32_t n_ground = 0u, n_nonground = 0u;
    constexpr int ITEMS = 4;
    for (int p0 = base; p0 < end; p0 += 64 * ITEMS) {
        uint32_t code[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) code[j] = split_code<MASKS>(row, min(p0 + j * 64 + lane, end - 1)); // (clamped: the loads do not wait for a test)
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const bool valid = p0 + j * 64 + lane < end;
            n_ground += (uint32_t)__popcll(__ballot(valid && code[j] == 1u));
            n_nonground += (uint32_t)__popcll(__ballot(valid && code[j] == 2u));
        }
    }
    if (lane == 0) x.chunk_counts[(size_t)io * x.nch + chunk] = make_uint2(n_ground, n_nonground); // (every chunk of every cloud: an empty one holds (0, 0))
}

template <int FMT, bool MASKS, bool HEIGHTS>
__global__ __launch_bounds__(256) void k_split_scatter(const Arena a, const SplitArgs x)
{
    const uint32_t item = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int cloud = (int)(item / gridDim.x), bx = (int)(item % gridDim.x);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = bx * 4 + wave;
    if (chunk >= x.nch) return; // (uniform over the wavefront; there is no barrier below)
    const SplitCloud &c = x.clouds[cloud];
    const int n = c.n_points, io = c.io_index;

    // the sets' sizes in front of this chunk; the first wavefront of a cloud goes on to the end and leaves the totals
    const uint2 *pairs = x.chunk_counts + (size_t)io * x.nch;
    uint32_t at[2] = {0u, 0u};
    for (int q = lane; q < chunk; q += 64) {
        const uint2 v = pairs[q];
        at[0] += v.x;
        at[1] += v.y;
    }
    at[0] = wave_sum(at[0]);
    at[1] = wave_sum(at[1]);
    if (chunk == 0) {
        uint32_t t0 = 0u, t1 = 0u;
        for (int q = lane; q < x.nch; q += 64) {
            const uint2 v = pairs[q];
            t0 += v.x;
            t1 += v.y;
        }
        t0 = wave_sum(t0);
        t1 = wave_sum(t1);
        if (lane == 0) {
            x.counts[(size_t)io * 2] = (int32_t)t0;
            x.counts[(size_t)io * 2 + 1] = (int32_t)t1;
        }
    }

    const int base = min(chunk * a.PW, n);
    const int end = min(base + a.PW, n);
    if (base >= end) return;
    const uint8_t *row = split_label_row<MASKS>(x, io);
    const uint4 *pts = reinterpret_cast<const uint4 *>(x.points) + (size_t)io * x.cloud_stride * (FMT == GG_POINT16 ? 1 : 2);
    const size_t out0 = (size_t)io * x.cloud_stride;
    const bool has_tf = c.has_tf != 0, fresh = c.fresh != 0;
    const float fresh_z = c.fresh_z;
    const double pos_x = c.pos_x, pos_y = c.pos_y;
    double tf[12];
    if (has_tf) { // (uniform)
#pragma unroll
        for (int k = 0; k < 12; ++k) tf[k] = c.tf[k];
    }
    const float2 *gp2 = gp2_ptr(a, c.slot);

    constexpr int ITEMS = 4;
    for (int p0 = base; p0 < end; p0 += 64 * ITEMS) {
        uint4 v[ITEMS];
        uint32_t ring[ITEMS], code[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) { // all windows' loads in flight together (unconditional, at clamped indices)
            const int p = min(p0 + j * 64 + lane, end - 1);
            code[j] = split_code<MASKS>(row, p);
            if (FMT == GG_POINT16) {
                v[j] = pts[p];
                ring[j] = v[j].w & 0xFFFFu;
            } else {
                v[j] = pts[(size_t)p * 2];                    // x, y, z, pad0
                ring[j] = pts[(size_t)p * 2 + 1].y & 0xFFFFu; // intensity, ring | pad1 << 16, pad2
            }
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int p = p0 + j * 64 + lane;
            const uint32_t sel = p < end ? code[j] : 0u;
            const unsigned long long m0 = __ballot(sel == 1u), m1 = __ballot(sel == 2u);
            const int s = sel == 2u ? 1 : 0;
            const uint32_t k = at[s] + (uint32_t)rank_below(s ? m1 : m0); // the point's place in its set: below the set's size, at most n_points <= cloud_stride
            if (sel && k < (uint32_t)n) { // (k >= n: the labels changed between the two launches -- nothing is written outside the row)
                const size_t o = out0 + k;
                const SplitSet &set = x.set[s];
                float px = __uint_as_float(v[j].x), py = __uint_as_float(v[j].y), pz = __uint_as_float(v[j].z);
                if (has_tf) transform_point(tf, px, py, pz);
                if (set.points) reinterpret_cast<uint4 *>(set.points)[o] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), ring[j]);
                if (set.source) set.source[o] = p;
                if (HEIGHTS && set.height) {
                    float h = __uint_as_float(0x7FC00000u); // a selected point outside the map: the caller's labels are not this cloud's
                    int r, cc;
                    const bool inside = position_inside(a.g, pos_x, pos_y, (double)px, (double)py);
                    index_from_position(a.g, pos_x, pos_y, (double)px, (double)py, r, cc);
                    if (inside && r >= 0 && cc >= 0 && r < a.g.rows && cc < a.g.cols) h = pz - (fresh ? fresh_z : gp2[gp_idx(a, r, cc)].x);
                    set.height[o] = h;
                }
            }
            at[0] += (uint32_t)__popcll(m0);
            at[1] += (uint32_t)__popcll(m1);
        }
    }
}

template <int FMT, bool MASKS> static void launch_split_scatter(const Arena &a, const SplitArgs &x, dim3 grid, hipStream_t s)
{
    if (x.set[0].height || x.set[1].height)
        hipLaunchKernelGGL((k_split_scatter<FMT, MASKS, true>), grid, dim3(256), 0, s, a, x);
    else
        hipLaunchKernelGGL((k_split_scatter<FMT, MASKS, false>), grid, dim3(256), 0, s, a, x);
}

void launch_split(const Arena &a, const SplitArgs &x, int n_clouds, hipStream_t s)
{
    const dim3 grid((x.nch + 3) / 4, n_clouds); // (one launch for the whole call, as K1 / K5 / K8 launch a batch)
    const bool masks = x.masks != nullptr;
    if (masks)
        hipLaunchKernelGGL((k_split_count<true>), grid, dim3(256), 0, s, a, x);
    else
        hipLaunchKernelGGL((k_split_count<false>), grid, dim3(256), 0, s, a, x);
    if (x.point_format == GG_POINT16) {
        if (masks) launch_split_scatter<GG_POINT16, true>(a, x, grid, s);
        else launch_split_scatter<GG_POINT16, false>(a, x, grid, s);
    } else {
        if (masks) launch_split_scatter<GG_POINT32, true>(a, x, grid, s);
        else launch_split_scatter<GG_POINT32, false>(a, x, grid, s);
    }
}

} // namespace gg
