// K6 -- output wire formats of the nodelet (src/GroundGridNodelet.cpp:211-291), produced on the device so that only what
// is subscribed to crosses PCIe:
//   * per-layer 8-bit image: grid_map::GridMapCvConverter::toImage<unsigned char, 1> (Nodelet.cpp:239) -- the layer
//     normalised between the min and max of its finite cells, NaN / inf cells left 0.  (cv::applyColorMap, :240, is an
//     OpenCV lookup table applied by the host afterwards.)
//   * the 32FC3 "terrain" image (Nodelet.cpp:247-268): (ground, 3x3 pointsRaw sum >= 27 ? 1 : 0, pointsRaw) per cell.
//   * the layers themselves as dense planes, and back: the cell-by-cell converter of every getter, setter and many-map call.
// Images are row-major (cv::Mat), layers column-major (Eigen): the kernels transpose through the index math.
#include "gg_device.h"

#include <float.h>
#include <algorithm>

namespace gg {

// min / max over the finite cells of a layer (Eigen minCoeffOfFinites / maxCoeffOfFinites); out[0] = min, out[1] = max
__global__ __launch_bounds__(1024) void k_minmax_finite(const float *__restrict__ layer, int C, float *__restrict__ out)
{
    __shared__ float smin[16], smax[16];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int k = threadIdx.x; k < C; k += 1024) {
        const float v = layer[k];
        if (isfinite(v)) {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = lo;
        smax[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lo = fminf(lo, smin[w]);
            hi = fmaxf(hi, smax[w]);
        }
        out[0] = lo;
        out[1] = hi;
    }
}

// GridMapCvConverter::toImage<unsigned char,1>: imageValue = (uchar)(((clamp(v, lo, hi) - lo) / (hi - lo)) * 255.f)
__global__ __launch_bounds__(256) void k_layer_to_u8(const float *__restrict__ layer, int rows, int cols, const float *__restrict__ bounds,
                                                     uint8_t *__restrict__ img)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= rows || j >= cols) return;
    const float lo = bounds[0], hi = bounds[1];
    img[(size_t)i * cols + j] = layer_value_to_u8(layer[(size_t)i + (size_t)j * rows], lo, hi);
}

// Nodelet.cpp:258-268; the reference reads block<3,3>(i-1, j-1) also on the border (UB): border cells get 0 for the flag.
__global__ __launch_bounds__(256) void k_terrain_image(const Arena a, int slot, float *__restrict__ img)
{
    const float2 *gp2 = gp2_ptr(a, slot);
    const float *percall = percall_ptr(a, slot);
    const int rows = a.g.rows, cols = a.g.cols;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= rows || j >= cols) return;
    float flag = 0.0f;
    // (pointsRaw is a sparse per-call layer: 0 outside the live half columns, gg_internal.h tile_live)
    auto raw_at = [&](int r, int c) { return cell_is_live(a, slot, r, c) ? percall[percall_index_of(a, PL_POINTSRAW, r, c)] : 0.0f; };
    if (i >= 1 && j >= 1 && i + 1 < rows && j + 1 < cols) {
        float e[9];
#pragma unroll
        for (int s = 0; s < 9; ++s) e[s] = raw_at(i - 1 + s % 3, j - 1 + s / 3);
        flag = tree9(e) >= 27.0f ? 1.0f : 0.0f;
    }
    float *px = img + ((size_t)i * cols + j) * 3;
    px[0] = gp2[gp_idx(a, i, j)].x;
    px[1] = flag;
    px[2] = raw_at(i, j);
}

// The host boundary of the layers, cell by cell: dense planes <-> the sheared (ground, confidence) pairs and the sparse per-call tile blocks,
// for the maps listed in x.maps (blockIdx.y = map).  The ONE such form: gg_get_layer, gg_get_layers, the image and message getters, the
// fused call's layer downloads and gg_set_layer are lists of one map (gg_context::d_slot_maps), variant 1 of gg_export_layers /
// gg_import_layers lists many.  The tiled kernels (k9_export.hip, k10_import.hip) are the other, independent route to the same planes.
constexpr unsigned PAIR_MASK = (1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH);
__device__ __forceinline__ int plane_index(unsigned mask, int layer) { return __popc(mask & ((1u << layer) - 1u)); }

// Layers -> planes in destination order: plane k = the k-th layer of x.mask in gg_layer order.  A per-call layer gives its stored values in
// the live half columns and the per-call reset value (:61-75) everywhere else (gg_internal.h tile_live); a fresh map gives the reset's pair
// and its layer is not read.  The cell's liveness, its place in the tile blocks and its element of the sheared layer are worked out once
// for all the planes.
__global__ __launch_bounds__(256) void k_export_gather(const Arena a, const PlaneArgs x)
{
    const ExportMap m = x.maps[blockIdx.y];
    const float *src = percall_ptr(a, m.slot);
    const float2 *gp2 = gp2_ptr(a, m.slot);
    const int rows = a.g.rows, cols = a.g.cols;
    float *out = x.planes + (size_t)blockIdx.y * (size_t)x.n_planes * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const bool any_percall = (x.mask & ~((1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH))) != 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.g.C; i += gridDim.x * blockDim.x) {
        const int r = row_major ? i / cols : i % rows, c = row_major ? i % cols : i / rows;
        bool live = false;
        size_t at = 0;
        if (any_percall) {
            live = cell_is_live(a, m.slot, r, c);
            at = percall_index_of(a, 0, r, c);
        }
        float2 g = make_float2(m.fresh_z, (float)0.0000001);
        if (!m.fresh && (x.mask & ((1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH)))) g = gp2[gp_idx(a, r, c)];
        int k = 0;
#pragma unroll
        for (int l = 0; l < GG_NUM_LAYERS; ++l) {
            if (!((x.mask >> l) & 1u)) continue; // (uniform)
            float v;
            if (l == GG_LAYER_GROUND) v = g.x;
            else if (l == GG_LAYER_GROUNDPATCH) v = g.y;
            else v = live ? src[at + (size_t)percall_position(l) * (TILE * TILE)] : layer_reset_value(l);
            out[(size_t)k * x.plane_stride + i] = v;
            ++k;
        }
    }
}
// (one map: min((C + 255) / 256, 2048) work-groups, what the single-map getters always launched)
static int cell_blocks(const Arena &a, int n_maps) { return std::min((a.g.C + 255) / 256, n_maps >= 64 ? 64 : 2048); }
void launch_planes_gather(const Arena &a, const PlaneArgs &x, int n_maps, hipStream_t s)
{
    hipLaunchKernelGGL(k_export_gather, dim3(cell_blocks(a, n_maps), n_maps), dim3(256), 0, s, a, x);
}

// Make the maps' per-call layers dense in place: the reset values into every dead half column ...
__global__ __launch_bounds__(256) void k_materialise_maps(const Arena a, const ExportMap *__restrict__ maps)
{
    const int slot = maps[blockIdx.y].slot;
    const int rows = a.g.rows;
    float *L = percall_ptr(a, slot);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.g.C; i += gridDim.x * blockDim.x) {
        if (cell_is_live(a, slot, i % rows, i / rows)) continue;
        const size_t at = percall_index_of(a, 0, i % rows, i / rows);
        for (int l = 0; l < GG_NUM_LAYERS; ++l)
            if (percall_position(l) >= 0) L[at + (size_t)percall_position(l) * (TILE * TILE)] = layer_reset_value(l);
    }
}
// ... and, in the launch behind it, every half column of those maps marked live.  Needed before ONE per-call layer is overwritten cell by
// cell (the liveness words are shared by the nine layers, and the cells of a tile are spread over many work-groups) and before
// gg_insert_cloud continues the recurrences in the layers.
__global__ __launch_bounds__(256) void k_live_all_maps(const Arena a, const ExportMap *__restrict__ maps)
{
    uint32_t *tile_live = a.tile_live + (size_t)maps[blockIdx.y].slot * a.tile_live_stride;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < a.g.T; t += gridDim.x * blockDim.x) tile_live[t] = 0xFFFFFFFFu;
}
void launch_materialise_maps(const Arena &a, const ExportMap *maps, int n_maps, hipStream_t s)
{
    hipLaunchKernelGGL(k_materialise_maps, dim3(cell_blocks(a, n_maps), n_maps), dim3(256), 0, s, a, maps);
    hipLaunchKernelGGL(k_live_all_maps, dim3((a.g.T + 255) / 256, n_maps), dim3(256), 0, s, a, maps);
}

// Planes -> layers in source order.  One component of the pair named on a real map: a 4-byte store, the other is not read; on a fresh map
// the pair, with the reset's constant for the other.  Per-call layers are overwritten in place: launch_planes_scatter makes them dense first.
__global__ __launch_bounds__(256) void k_import_scatter(const Arena a, const PlaneArgs x)
{
    const ExportMap m = x.maps[blockIdx.y];
    float *dst = percall_ptr(a, m.slot);
    float2 *gp2 = gp2_ptr(a, m.slot);
    float *gpf = reinterpret_cast<float *>(gp2);
    const int rows = a.g.rows, cols = a.g.cols;
    const float *in = x.planes + (size_t)blockIdx.y * (size_t)x.n_planes * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const unsigned gp_mask = x.mask & PAIR_MASK;
    const bool any_percall = (x.mask & ~PAIR_MASK) != 0u;
    const float *in_conf = in + (size_t)plane_index(x.mask, GG_LAYER_GROUNDPATCH) * x.plane_stride;
    const float *in_ground = in + (size_t)plane_index(x.mask, GG_LAYER_GROUND) * x.plane_stride;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.g.C; i += gridDim.x * blockDim.x) {
        const int r = row_major ? i / cols : i % rows, c = row_major ? i % cols : i / rows;
        if (gp_mask) {
            const int e = gp_idx(a, r, c);
            if (gp_mask == PAIR_MASK) gp2[e] = make_float2(in_ground[i], in_conf[i]);
            else if (m.fresh) gp2[e] = gp_mask == (1u << GG_LAYER_GROUND) ? make_float2(in_ground[i], (float)0.0000001) : make_float2(m.fresh_z, in_conf[i]);
            else if (gp_mask == (1u << GG_LAYER_GROUND)) gpf[(size_t)e * 2] = in_ground[i];
            else gpf[(size_t)e * 2 + 1] = in_conf[i];
        }
        if (!any_percall) continue;
        const size_t at = percall_index_of(a, 0, r, c);
        int k = 0;
#pragma unroll
        for (int l = 0; l < GG_NUM_LAYERS; ++l) {
            if (!((x.mask >> l) & 1u)) continue; // (uniform)
            if (percall_position(l) >= 0) dst[at + (size_t)percall_position(l) * (TILE * TILE)] = in[(size_t)k * x.plane_stride + i];
            ++k;
        }
    }
}
void launch_planes_scatter(const Arena &a, const PlaneArgs &x, int n_maps, hipStream_t s)
{
    if (x.mask & ~PAIR_MASK) launch_materialise_maps(a, x.maps, n_maps, s);
    hipLaunchKernelGGL(k_import_scatter, dim3(cell_blocks(a, n_maps), n_maps), dim3(256), 0, s, a, x);
}

// GroundGrid's initial values (src/GroundGrid.cpp:71-75) into every per-call layer of n slots: element e of a slot's region belongs
// to layer position (e / 256) % 9
struct PercallInit {
    float v[PERCALL_LAYERS];
};
__global__ __launch_bounds__(256) void k_fill_percall(float *__restrict__ dst, size_t n, size_t stride, const PercallInit init)
{
    float *d = dst + (size_t)blockIdx.y * stride;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = init.v[(i / (TILE * TILE)) % PERCALL_LAYERS];
}
void launch_fill_percall(const Arena &a, int first_slot, int n_slots, const float init[GG_NUM_LAYERS], hipStream_t s)
{
    if (n_slots <= 0) return;
    PercallInit pi;
    for (int l = 0; l < GG_NUM_LAYERS; ++l)
        if (percall_position(l) >= 0) pi.v[percall_position(l)] = init[l];
    const size_t n = (size_t)a.g.T * PERCALL_BLOCK;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, n_slots >= 64 ? (size_t)64 : (size_t)1024);
    hipLaunchKernelGGL(k_fill_percall, dim3(blocks, n_slots), dim3(256), 0, s, percall_ptr(a, first_slot), n, a.slot_layer_stride, pi);
}

void launch_layer_to_u8(const float *layer, int rows, int cols, float *d_bounds, uint8_t *d_img, hipStream_t s)
{
    hipLaunchKernelGGL(k_minmax_finite, dim3(1), dim3(1024), 0, s, layer, rows * cols, d_bounds);
    dim3 grid((cols + 63) / 64, (rows + 3) / 4);
    hipLaunchKernelGGL(k_layer_to_u8, grid, dim3(256), 0, s, layer, rows, cols, d_bounds, d_img);
}

void launch_terrain_image(const Arena &a, int slot, float *d_img, hipStream_t s)
{
    dim3 grid((a.g.cols + 63) / 64, (a.g.rows + 3) / 4);
    hipLaunchKernelGGL(k_terrain_image, grid, dim3(256), 0, s, a, slot, d_img);
}

} // namespace gg
