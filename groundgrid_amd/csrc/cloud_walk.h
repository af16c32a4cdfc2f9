// cloud_walk.h -- the one walk over a batch of labelled clouds: what k12_split.hip, k13_raster.hip and k15_cluster.hip share.
//
// A call covers the clouds of a CloudArgs in a.PW-point chunks, one wavefront per chunk and four wavefronts per work-group, grid
// (ceil(nch / 4), clouds) under xcd_contiguous_item (the chunks of a cloud share an L2).  A kernel is
//   CloudChunk k;
//   if (!cloud_chunk(a, x.cl, k)) return;       // this wavefront has no chunk (uniform)
//   ... what it owes even an empty chunk (k_split_count's pair, k_split_scatter's prefix sums and totals) ...
//   if (k.base >= k.end) return;                // left to the kernel for that reason
//   CloudFrame f;
//   load_cloud_frame(a, x.cl.clouds[k.cloud], f);
//   walk_chunk<FMT, MASKS, WALK_...>(x.cl, k, [&](int p, uint32_t code, const uint4 &v, uint32_t ring) GG_INLINE_LAMBDA { ... });
// and its body sees one point per lane: locate_point, height_above_ground, linear_cell.
//
// THE CONVERGENCE CONTRACT.  walk_chunk calls the body once per 64-point window with ALL 64 lanes active and in wavefront-uniform control
// flow, also for the lanes behind the chunk's end (their code is 0, their words are those of the chunk's last point: the loads are
// unconditional at clamped indices).  Bodies use __ballot and __shfl (k_split_count, k_split_scatter, the IDS pass of k_cluster_points), so
//   - nothing between the kernel's entry and walk_chunk may make lanes of a wavefront leave or diverge, and
//   - a body may not `return` (or otherwise branch) around a ballot or shuffle on a condition that differs between lanes: such a return
//     takes lanes out of the next cross-lane operation of the SAME call.  A lane-dependent early return is fine in a body without cross-lane
//     operations (k_raster_scatter, the COUNT pass), a wavefront-uniform one anywhere.
// The body is forced inline (GG_INLINE_LAMBDA) and takes the frame by reference, so a cloud's uniform values stay in scalar registers.
#pragma once

#include <type_traits>

#include "gg_device.h"

namespace gg {

#define GG_INLINE_LAMBDA __attribute__((always_inline))

constexpr uint32_t QUIET_NAN_BITS = 0x7FC00000u; // "no such point": a height outside the map, an extreme of no point

// The order-preserving key of a height: key(h) = bits(h) ^ (sign(h) ? 0xFFFFFFFF : 0x80000000) orders the non-NaN floats as IEEE totalOrder
// does (-0.0 below +0.0, the infinities at the ends) and maps none of them to 0 or to 0xFFFFFFFF (those would be the bits 0xFFFFFFFF and
// 0x7FFFFFFF, both NaNs): the two values mark "no point yet" under an integer atomicMax / atomicMin.
GG_DEV uint32_t height_key(float h)
{
    const uint32_t b = __float_as_uint(h);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
GG_DEV uint32_t height_of_key(uint32_t key) { return (key >> 31) ? key ^ 0x80000000u : ~key; }

GG_DEV uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
GG_DEV int wave_min_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
GG_DEV int wave_max_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
GG_DEV uint32_t wave_max_u(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

// The (cloud, chunk) of this wavefront and the chunk's points [base, end) of the cloud's n; io: the cloud's row of the caller's buffers
struct CloudChunk {
    int cloud, chunk, lane, n, io, base, end;
};
GG_DEV bool cloud_chunk(const Arena &a, const CloudArgs &x, CloudChunk &k)
{
    const uint32_t item = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int bx = (int)(item % gridDim.x);
    k.cloud = (int)(item / gridDim.x);
    k.chunk = bx * 4 + (int)(threadIdx.x >> 6);
    k.lane = threadIdx.x & 63;
    if (k.chunk >= x.nch) return false; // (uniform over the wavefront)
    k.n = x.clouds[k.cloud].n_points;
    k.io = x.clouds[k.cloud].io_index;
    k.base = min(k.chunk * a.PW, k.n);
    k.end = min(k.base + a.PW, k.n);
    return true;
}

// What every point of a cloud shares (uniform over the work-group); tf is loaded only when has_tf
struct CloudFrame {
    bool has_tf, fresh;
    float fresh_z;
    double pos_x, pos_y;
    double tf[12];
    const float2 *gp2;
};
GG_DEV void load_cloud_frame(const Arena &a, const SplitCloud &c, CloudFrame &f)
{
    f.has_tf = c.has_tf != 0;
    f.fresh = c.fresh != 0;
    f.fresh_z = c.fresh_z;
    f.pos_x = c.pos_x;
    f.pos_y = c.pos_y;
    if (f.has_tf) { // (uniform)
#pragma unroll
        for (int k = 0; k < 12; ++k) f.tf[k] = c.tf[k];
    }
    f.gp2 = gp2_ptr(a, c.slot);
}

// what walk_chunk loads per point: its label code alone; with its first 16 bytes (x, y, z, and ring | pad0 or pad0); with its ring too (GG_POINT32 reads its second 16 bytes for it)
enum : int { WALK_CODE = 0, WALK_POINT = 1, WALK_POINT_RING = 2 };

// The chunk in 64-point windows, four windows' loads in flight together; body(p, code, v, ring) per window under the contract above: p the
// lane's point index (>= k.end behind the chunk), code its split_code or 0 behind the chunk, v and ring as LOAD says (else zero).
template <int FMT, bool MASKS, int LOAD, class Body> GG_DEV void walk_chunk(const CloudArgs &x, const CloudChunk &k, Body &&body)
{
    const uint8_t *row = MASKS ? x.masks + (size_t)k.io * ((x.cloud_stride + 3) / 4) : x.labels + (size_t)k.io * x.cloud_stride;
    const uint4 *pts = reinterpret_cast<const uint4 *>(x.points) + (size_t)k.io * x.cloud_stride * (FMT == GG_POINT16 ? 1 : 2);
    constexpr int ITEMS = 4;
    for (int p0 = k.base; p0 < k.end; p0 += 64 * ITEMS) {
        uint4 v[ITEMS];
        uint32_t ring[ITEMS], code[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) { // (unconditional, at clamped indices: the loads do not wait for a test)
            const int p = min(p0 + j * 64 + k.lane, k.end - 1);
            code[j] = split_code<MASKS>(row, p);
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            ring[j] = 0u;
            if (LOAD != WALK_CODE) v[j] = pts[FMT == GG_POINT16 ? (size_t)p : (size_t)p * 2];
            if (LOAD == WALK_POINT_RING) ring[j] = (FMT == GG_POINT16 ? v[j].w : pts[(size_t)p * 2 + 1].y) & 0xFFFFu; // (intensity, ring | pad1 << 16, pad2)
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int p = p0 + j * 64 + k.lane;
            body(p, p < k.end ? code[j] : 0u, v[j], ring[j]);
        }
    }
}

// a point of the cloud in the map's frame
GG_DEV void to_map_frame(const CloudFrame &f, float &px, float &py, float &pz)
{
    if (f.has_tf) transform_point(f.tf, px, py, pz);
}
// THE inside-the-map test: the cell (r, cc) a map-frame point lands in, false when it lands in none
GG_DEV bool cell_of_point(const Arena &a, const CloudFrame &f, float px, float py, int &r, int &cc)
{
    const bool inside = position_inside(a.g, f.pos_x, f.pos_y, (double)px, (double)py);
    index_from_position(a.g, f.pos_x, f.pos_y, (double)px, (double)py, r, cc);
    return inside && r >= 0 && cc >= 0 && r < a.g.rows && cc < a.g.cols;
}
GG_DEV bool locate_point(const Arena &a, const CloudFrame &f, float &px, float &py, float &pz, int &r, int &cc)
{
    to_map_frame(f, px, py, pz);
    return cell_of_point(a, f, px, py, r, cc);
}
// the ground under (r, cc) is gathered here and nowhere else
GG_DEV float height_above_ground(const Arena &a, const CloudFrame &f, float pz, int r, int cc) { return pz - (f.fresh ? f.fresh_z : f.gp2[gp_idx(a, r, cc)].x); }
// the linear cell of `order`: < rows * cols <= plane_stride
GG_DEV int linear_cell(const Arena &a, bool row_major, int r, int cc) { return row_major ? r * a.g.cols + cc : r + cc * a.g.rows; }

// (point_format, masks or labels) as the <FMT, MASKS> of a launch: f(fmt, masks) with two std::integral_constant arguments
template <class F> static void dispatch_cloud_variant(const CloudArgs &x, F &&f)
{
    using P16 = std::integral_constant<int, GG_POINT16>;
    using P32 = std::integral_constant<int, GG_POINT32>;
    if (x.point_format == GG_POINT16) {
        if (x.masks) f(P16{}, std::true_type{});
        else f(P16{}, std::false_type{});
    } else {
        if (x.masks) f(P32{}, std::true_type{});
        else f(P32{}, std::false_type{});
    }
}

} // namespace gg
