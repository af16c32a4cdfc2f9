// K12 -- gg_split_clouds: the ground and the non-ground points of MANY labelled clouds as dense clouds in device memory, with every point's
// height above the estimated terrain and its index in the input cloud (include/groundgrid_hip.h).  What a consumer behind the segmenter
// gets today with `points[labels == 99]` per cloud -- a launch and a device -> host synchronisation per cloud, the output size being data
// dependent -- in two launches for the whole batch and with the counts left on the device.
//
// Both launches walk the clouds as cloud_walk.h describes (one wavefront per a.PW-point chunk; their bodies hold to its convergence contract):
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
#include "cloud_walk.h"

namespace gg {

template <bool MASKS>
__global__ __launch_bounds__(256) void k_split_count(const Arena a, const SplitArgs x)
{
    CloudChunk k;
    if (!cloud_chunk(a, x.cl, k)) return;
    uint32_t n_ground = 0u, n_nonground = 0u;
    walk_chunk<GG_POINT16, MASKS, WALK_CODE>(x.cl, k, [&](int, uint32_t code, const uint4 &, uint32_t) GG_INLINE_LAMBDA {
        n_ground += (uint32_t)__popcll(__ballot(code == 1u));
        n_nonground += (uint32_t)__popcll(__ballot(code == 2u));
    });
    if (k.lane == 0) x.chunk_counts[(size_t)k.io * x.cl.nch + k.chunk] = make_uint2(n_ground, n_nonground); // (every chunk of every cloud: an empty one holds (0, 0))
}

template <int FMT, bool MASKS, bool HEIGHTS>
__global__ __launch_bounds__(256) void k_split_scatter(const Arena a, const SplitArgs x)
{
    CloudChunk k;
    if (!cloud_chunk(a, x.cl, k)) return; // (there is no barrier below)
    const int lane = k.lane, n = k.n;

    // the sets' sizes in front of this chunk; the first wavefront of a cloud goes on to the end and leaves the totals
    const uint2 *pairs = x.chunk_counts + (size_t)k.io * x.cl.nch;
    uint32_t at[2] = {0u, 0u};
    for (int q = lane; q < k.chunk; q += 64) {
        const uint2 v = pairs[q];
        at[0] += v.x;
        at[1] += v.y;
    }
    at[0] = wave_sum(at[0]);
    at[1] = wave_sum(at[1]);
    if (k.chunk == 0) {
        uint32_t t0 = 0u, t1 = 0u;
        for (int q = lane; q < x.cl.nch; q += 64) {
            const uint2 v = pairs[q];
            t0 += v.x;
            t1 += v.y;
        }
        t0 = wave_sum(t0);
        t1 = wave_sum(t1);
        if (lane == 0) {
            x.counts[(size_t)k.io * 2] = (int32_t)t0;
            x.counts[(size_t)k.io * 2 + 1] = (int32_t)t1;
        }
    }

    if (k.base >= k.end) return;
    const size_t out0 = (size_t)k.io * x.cl.cloud_stride;
    CloudFrame f;
    load_cloud_frame(a, x.cl.clouds[k.cloud], f);
    walk_chunk<FMT, MASKS, WALK_POINT_RING>(x.cl, k, [&](int p, uint32_t sel, const uint4 &v, uint32_t ring) GG_INLINE_LAMBDA {
        const unsigned long long m0 = __ballot(sel == 1u), m1 = __ballot(sel == 2u);
        const int s = sel == 2u ? 1 : 0;
        const uint32_t place = at[s] + (uint32_t)rank_below(s ? m1 : m0); // the point's place in its set: below the set's size, at most n_points <= cloud_stride
        if (sel && place < (uint32_t)n) { // (place >= n: the labels changed between the two launches -- nothing is written outside the row)
            const size_t o = out0 + place;
            const SplitSet &set = x.set[s];
            float px = __uint_as_float(v.x), py = __uint_as_float(v.y), pz = __uint_as_float(v.z);
            to_map_frame(f, px, py, pz);
            if (set.points) reinterpret_cast<uint4 *>(set.points)[o] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), ring);
            if (set.source) set.source[o] = p;
            if (HEIGHTS && set.height) {
                int r, cc; // a selected point outside the map: the caller's labels are not this cloud's
                set.height[o] = cell_of_point(a, f, px, py, r, cc) ? height_above_ground(a, f, pz, r, cc) : __uint_as_float(QUIET_NAN_BITS);
            }
        }
        at[0] += (uint32_t)__popcll(m0);
        at[1] += (uint32_t)__popcll(m1);
    });
}

void launch_split(const Arena &a, const SplitArgs &x, int n_clouds, hipStream_t s)
{
    const dim3 grid((x.cl.nch + 3) / 4, n_clouds); // (one launch for the whole call, as K1 / K5 / K8 launch a batch)
    dispatch_cloud_variant(x.cl, [&](auto fmt, auto masks) {
        constexpr int FMT = decltype(fmt)::value;
        constexpr bool MASKS = decltype(masks)::value;
        hipLaunchKernelGGL((k_split_count<MASKS>), grid, dim3(256), 0, s, a, x);
        if (x.set[0].height || x.set[1].height)
            hipLaunchKernelGGL((k_split_scatter<FMT, MASKS, true>), grid, dim3(256), 0, s, a, x);
        else
            hipLaunchKernelGGL((k_split_scatter<FMT, MASKS, false>), grid, dim3(256), 0, s, a, x);
    });
}

} // namespace gg
