// K13 -- gg_rasterize_clouds: the obstacle grid of MANY labelled clouds as dense planes in device memory (include/groundgrid_hip.h): per cell
// of a cloud's map the number of its non-ground (ground) points there and the largest and the smallest height of them above the estimated
// terrain.  What a caller composes today from gg_split_clouds and a scatter-reduce over cell indices it computes itself, in one pass over
// the points and with the library's own inside test and index arithmetic.
//
// Nothing depends on the order in which points arrive: a count is an integer atomic add, a height an integer atomic max / min on its
// height_key (cloud_walk.h), which is never 0 or 0xFFFFFFFF: the two values mark "no point yet".  No float is added.
// Three launches on the caller's planes, no scratch:
//   k_raster_planes<false>  every word of every named plane := 0 (a count, a max key) or 0xFFFFFFFF (a min key); 16-byte stores.
//   k_raster_scatter        the walk of cloud_walk.h (one wavefront per a.PW-point chunk); per selected point inside the map at most one
//                           atomic add, one atomic max and one atomic min into its cloud's planes, none of them returning a value.  The
//                           ground under a point is gathered only where a height channel of its set is named.
//   k_raster_planes<true>   in place: a counter becomes its float, a key its float or the quiet NaN 0x7FC00000 where it still holds the
//                           initial value.
// No work-group waits for another, and nothing a batch left behind is read.
//
// Algorithmic bytes: per input point 1 (labels; 0.25 with masks) + 16 (32: GG_POINT32); per selected point inside the map 8 gathered (the
// (ground, confidence) pair, height channels only) and one 4-byte atomic per named channel of its set; per cell and named plane 4 written by
// the first launch and 4 read + 4 written by the third.
#include "cloud_walk.h"

namespace gg {

// kind of a channel: 0 count, 1 max height, 2 min height (GG_RASTER_* come as two such triples)
GG_DEV uint32_t raster_initial_word(int kind) { return kind == 2 ? 0xFFFFFFFFu : 0u; }
GG_DEV uint32_t raster_final_word(int kind, uint32_t w)
{
    if (kind == 0) return __float_as_uint((float)w);
    return w == raster_initial_word(kind) ? QUIET_NAN_BITS : height_of_key(w);
}

// Every word of every named plane once, one plane per `parts` consecutive work-groups: 16-byte accesses over the 16-byte aligned body of the
// plane's rows * cols words, single words in front of it and behind it (d_dst and plane_stride promise 4-byte alignment only).
template <bool FINAL>
__global__ __launch_bounds__(256) void k_raster_planes(const Arena a, const RasterArgs x, int parts)
{
    const int plane = (int)(blockIdx.x / (uint32_t)parts);
    const int v = (int)(blockIdx.x % (uint32_t)parts) * 256 + (int)threadIdx.x;
    int channel = 0;
    for (int k = plane % x.n_planes; channel < GG_NUM_RASTER_CHANNELS; ++channel) // the k-th named channel (uniform)
        if (((x.channel_mask >> channel) & 1u) && k-- == 0) break;
    const int kind = channel % 3;
    uint32_t *p = x.planes + (size_t)plane * x.plane_stride;
    const int C = a.g.C;
    const int lead = min(C, (int)(((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u) >> 2));
    const int nvec = (C - lead) >> 2;
    const int tail = lead + 4 * nvec; // first word behind the body
    const uint32_t w0 = raster_initial_word(kind);
    if (v < nvec) {
        uint4 *q = reinterpret_cast<uint4 *>(p + lead) + v;
        uint4 w = make_uint4(w0, w0, w0, w0);
        if (FINAL) {
            w = *q;
            w = make_uint4(raster_final_word(kind, w.x), raster_final_word(kind, w.y), raster_final_word(kind, w.z), raster_final_word(kind, w.w));
        }
        *q = w;
    }
    if (v < lead) p[v] = FINAL ? raster_final_word(kind, p[v]) : w0;
    if (v < C - tail) p[tail + v] = FINAL ? raster_final_word(kind, p[tail + v]) : w0;
}

template <int FMT, bool MASKS, bool HEIGHTS>
__global__ __launch_bounds__(256) void k_raster_scatter(const Arena a, const RasterArgs x)
{
    CloudChunk k;
    if (!cloud_chunk(a, x.cl, k) || k.base >= k.end) return; // (uniform over the wavefront; there is no barrier below)
    uint32_t *planes = x.planes + (size_t)k.io * x.n_planes * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    CloudFrame f;
    load_cloud_frame(a, x.cl.clouds[k.cloud], f);
    walk_chunk<FMT, MASKS, WALK_POINT>(x.cl, k, [&](int, uint32_t sel, const uint4 &v, uint32_t) GG_INLINE_LAMBDA { // (no cross-lane operation: the returns are free)
        // the planes of the point's set (-1: not named)
        const int k_count = sel == 2u ? x.plane_of[GG_RASTER_NONGROUND_COUNT] : x.plane_of[GG_RASTER_GROUND_COUNT];
        const int k_max = sel == 2u ? x.plane_of[GG_RASTER_NONGROUND_MAX_HEIGHT] : x.plane_of[GG_RASTER_GROUND_MAX_HEIGHT];
        const int k_min = sel == 2u ? x.plane_of[GG_RASTER_NONGROUND_MIN_HEIGHT] : x.plane_of[GG_RASTER_GROUND_MIN_HEIGHT];
        if (!sel || (k_count & k_max & k_min) < 0) return; // (all three -1)
        float px = __uint_as_float(v.x), py = __uint_as_float(v.y), pz = __uint_as_float(v.z);
        int r, cc;
        if (!locate_point(a, f, px, py, pz, r, cc)) return; // the caller's labels are not this cloud's: nothing is touched
        const int cell = linear_cell(a, row_major, r, cc);
        if (k_count >= 0) atomicAdd(planes + (size_t)k_count * x.plane_stride + cell, 1u);
        if (HEIGHTS && (k_max & k_min) >= 0) {
            const float h = height_above_ground(a, f, pz, r, cc);
            if (h == h) { // (a NaN height is counted and takes part in neither extreme)
                const uint32_t key = height_key(h);
                if (k_max >= 0) atomicMax(planes + (size_t)k_max * x.plane_stride + cell, key);
                if (k_min >= 0) atomicMin(planes + (size_t)k_min * x.plane_stride + cell, key);
            }
        }
    });
}

void launch_raster(const Arena &a, const RasterArgs &x, int n_clouds, hipStream_t s)
{
    const int parts = (a.g.C / 4 + 1 + 255) / 256; // threads per plane: its 16-byte body, and at least the three single words at either end
    const dim3 plane_grid((uint32_t)parts * (uint32_t)(n_clouds * x.n_planes));
    hipLaunchKernelGGL((k_raster_planes<false>), plane_grid, dim3(256), 0, s, a, x, parts);
    const dim3 grid((x.cl.nch + 3) / 4, n_clouds);
    constexpr unsigned heights = (1u << GG_RASTER_NONGROUND_MAX_HEIGHT) | (1u << GG_RASTER_NONGROUND_MIN_HEIGHT) | (1u << GG_RASTER_GROUND_MAX_HEIGHT) |
                                 (1u << GG_RASTER_GROUND_MIN_HEIGHT);
    dispatch_cloud_variant(x.cl, [&](auto fmt, auto masks) {
        constexpr int FMT = decltype(fmt)::value;
        constexpr bool MASKS = decltype(masks)::value;
        if (x.channel_mask & heights)
            hipLaunchKernelGGL((k_raster_scatter<FMT, MASKS, true>), grid, dim3(256), 0, s, a, x);
        else // (a count-only call gathers no ground)
            hipLaunchKernelGGL((k_raster_scatter<FMT, MASKS, false>), grid, dim3(256), 0, s, a, x);
    });
    hipLaunchKernelGGL((k_raster_planes<true>), plane_grid, dim3(256), 0, s, a, x, parts);
}

} // namespace gg
