// K14 -- gg_export_slopes: the SHAPE of the terrain of many maps as dense planes in device memory, one launch (include/groundgrid_hip.h,
// where the six channels are defined to the bit: gradient in x and y, tangent, normal z, step, minimum confidence over the clamped 3 x 3
// neighbourhood of every cell).
//
// k_slopes_tiled has the shape of k_export_tiled (k9_export.hip): a work-group owns one 64 x 64 block of one map, reads the block's (ground,
// confidence) pairs in ELEMENT order through the export table -- consecutive lanes read consecutive elements of the sheared layer wherever
// the layout has them --, stages them in LDS and writes every named plane in runs of 64 consecutive floats (256 bytes per wavefront store)
// for either order; the row-major planes are the transposed read of the same LDS block.  What K14 adds:
//   * the one-cell HALO of the block: at most 4 * 64 + 4 = 260 cells, gathered through gp_idx.  Only halo cells INSIDE the map are addressed
//     (in the layer and in LDS alike): the clamped indices of the definition never leave the map, so a cell on the map's border reads its own
//     row / column in place of the missing one and the LDS words of the missing halo are never read.
//   * the LDS block is 66 x 66 per component, cell (ri, ci) of the block (-1 .. 64) at (ri + 1) + (ci + 1) * SL_LD with SL_LD = 67.  Every
//     access of the compute loop is a 4-byte ds_read, whose banks are (address / 4) mod 32 within each half of a wavefront.  A wavefront
//     holds 64 consecutive ri of one ci (column-major planes: stride 1) or 64 consecutive ci of one ri (row-major: stride SL_LD).  Stride 1
//     puts the 32 lanes of a half on 32 different banks; stride SL_LD does so exactly when SL_LD is odd (an odd number is a unit mod 32), and
//     66 is the smallest pitch that holds the block, so 67.  The eight neighbour reads are the same two walks shifted by a constant -- except
//     on the map's border, where the lanes of a clamped row share their centre's address (a broadcast or a neighbouring bank, at worst a
//     2-way conflict for the one wavefront in a block that holds the seam between clamped and unclamped lanes).
//   * the confidence component is staged (and read from memory) only when MIN_CONFIDENCE is named.
//   * every cell is computed ONCE: the 3 x 3 neighbourhood comes out of LDS into registers, the named channels are computed from it and each
//     goes to its plane with a single-word store (the plane base is only 4-byte aligned).
// A fresh map (gg_reset_maps left its layer unwritten) gets the constants of a level plane; neither its layer nor LDS is touched.
// No atomics, no scratch.
//
// k_slopes_gather is the cell-by-cell form: every thread takes one destination cell and gathers its up to nine pairs through gp_idx.
// gg_debug_set_tuning "slopes_variant" = 1 runs gg_export_slopes through it (the A/B of tools/bench_slopes.py and the in-library cross-check).
#include "gg_device.h"

#include <algorithm>

namespace gg {

constexpr int SL_LD = EXPORT_TILE + 3;                 // LDS pitch (above)
constexpr int SL_WORDS = (EXPORT_TILE + 2) * SL_LD;    // one component of a block with its halo
constexpr int SL_HALO = 4 * EXPORT_TILE + 4;
constexpr float SL_FRESH_CONFIDENCE = (float)0.0000001; // (gg_context::fresh: what the reset writes)

__device__ __forceinline__ int slope_plane_index(unsigned mask, int channel) { return __popc(mask & ((1u << channel) - 1u)); }

// The definition, on the clamped neighbourhood of one cell: g / w [(dr + 1) + 3 * (dc + 1)] is the cell at (row + dr, column + dc) with
// row - 1 / row + 1 / column - 1 / column + 1 replaced by row / column where they leave the map (a cell then stands in the array twice,
// which changes no maximum and no minimum); span_r = r_hi - r_lo, span_c = c_hi - c_lo.  `w` is read only with MIN_CONFIDENCE in the mask.
__device__ __forceinline__ void slope_cell(const float g[9], const float w[9], int span_r, int span_c, float res, unsigned mask, float v[GG_NUM_SLOPE_CHANNELS])
{
    const float gx = (g[3] - g[5]) / ((float)span_r * res);
    const float gy = (g[1] - g[7]) / ((float)span_c * res);
    const float s = gx * gx + gy * gy;
    v[GG_SLOPE_GRAD_X] = gx;
    v[GG_SLOPE_GRAD_Y] = gy;
    v[GG_SLOPE_TANGENT] = sqrtf(s);
    v[GG_SLOPE_NORMAL_Z] = 1.0f / sqrtf(s + 1.0f);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (k != 4) m = fmaxf(m, fabsf(g[k] - g[4]));
    v[GG_SLOPE_STEP] = m;
    float lo = 0.0f;
    if (mask & (1u << GG_SLOPE_MIN_CONFIDENCE)) { // (uniform)
        lo = w[4];
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k != 4) lo = fminf(lo, w[k]);
    }
    v[GG_SLOPE_MIN_CONFIDENCE] = lo;
}

__device__ __forceinline__ void fresh_values(float v[GG_NUM_SLOPE_CHANNELS])
{
    v[GG_SLOPE_GRAD_X] = 0.0f;
    v[GG_SLOPE_GRAD_Y] = 0.0f;
    v[GG_SLOPE_TANGENT] = 0.0f;
    v[GG_SLOPE_NORMAL_Z] = 1.0f;
    v[GG_SLOPE_STEP] = 0.0f;
    v[GG_SLOPE_MIN_CONFIDENCE] = SL_FRESH_CONFIDENCE;
}

// x.mask: bit per GG_SLOPE_*; everything else of PlaneArgs as for the export
__global__ __launch_bounds__(256) void k_slopes_tiled(const Arena a, const PlaneArgs x)
{
    __shared__ float lds[2][SL_WORDS];
    const int tid = threadIdx.x;
    const ExportMap m = x.maps[blockIdx.y];
    const int mt = (int)blockIdx.x, mtr = mt % x.blocks_r, mtc = mt / x.blocks_r;
    const int r0 = mtr * EXPORT_TILE, c0 = mtc * EXPORT_TILE;
    const int rows = a.g.rows, cols = a.g.cols;
    const int nr = min(EXPORT_TILE, rows - r0), nc = min(EXPORT_TILE, cols - c0);
    float *out = x.planes + (size_t)blockIdx.y * (size_t)x.n_planes * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const unsigned mask = x.mask;
    const bool want_conf = (mask & (1u << GG_SLOPE_MIN_CONFIDENCE)) != 0u;
    const float res = a.g.resolution_f;

    if (!m.fresh) {
        const float2 *gp2 = gp2_ptr(a, m.slot);
        const float *gpf = reinterpret_cast<const float *>(gp2);
        // the block, in element order
        const uint32_t first = x.block_off[mt], end = x.block_off[mt + 1];
        for (uint32_t i = first + tid; i < end; i += 256) {
            const uint32_t e = x.elem[i], c = x.cell[i]; // row in block | column in block << 6
            const int at = (int)(c & 63u) + 1 + ((int)(c >> 6) + 1) * SL_LD;
            if (want_conf) {
                const float2 v = gp2[e];
                lds[0][at] = v.x;
                lds[1][at] = v.y;
            } else {
                lds[0][at] = gpf[2 * (size_t)e];
            }
        }
        // its halo: the rows above and below (corners included), then the columns left and right
        for (int h = tid; h < SL_HALO; h += 256) {
            int ri, ci;
            if (h < 2 * (EXPORT_TILE + 2)) {
                const bool below = h >= EXPORT_TILE + 2;
                ri = below ? nr : -1;
                ci = h - (below ? EXPORT_TILE + 2 : 0) - 1; // -1 .. 64
                if (ci > nc) continue;
            } else {
                const int k = h - 2 * (EXPORT_TILE + 2);
                const bool right = k >= EXPORT_TILE;
                ci = right ? nc : -1;
                ri = k - (right ? EXPORT_TILE : 0); // 0 .. 63
                if (ri >= nr) continue;
            }
            const int r = r0 + ri, c = c0 + ci;
            if (r < 0 || r >= rows || c < 0 || c >= cols) continue; // (outside the map: never addressed, never read below)
            const int e = gp_idx(a, r, c), at = (ri + 1) + (ci + 1) * SL_LD;
            if (want_conf) {
                const float2 v = gp2[e];
                lds[0][at] = v.x;
                lds[1][at] = v.y;
            } else {
                lds[0][at] = gpf[2 * (size_t)e];
            }
        }
        __syncthreads();
    }

    float *plane[GG_NUM_SLOPE_CHANNELS];
#pragma unroll
    for (int k = 0; k < GG_NUM_SLOPE_CHANNELS; ++k) plane[k] = out + (size_t)slope_plane_index(mask, k) * x.plane_stride;

    // the block -> the named planes: a wavefront covers 64 consecutive floats of a plane in either order
#pragma unroll 2
    for (int idx = tid; idx < EXPORT_TILE * EXPORT_TILE; idx += 256) {
        const int fast = idx & (EXPORT_TILE - 1), slow = idx >> 6;
        const int ri = row_major ? slow : fast, ci = row_major ? fast : slow;
        if (ri >= nr || ci >= nc) continue;
        const int r = r0 + ri, c = c0 + ci;
        float v[GG_NUM_SLOPE_CHANNELS];
        if (m.fresh) { // (uniform)
            fresh_values(v);
        } else {
            const int dr[3] = {r > 0 ? -1 : 0, 0, r < rows - 1 ? 1 : 0};
            const int dc[3] = {c > 0 ? -SL_LD : 0, 0, c < cols - 1 ? SL_LD : 0};
            const int at = (ri + 1) + (ci + 1) * SL_LD;
            float g[9], w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                g[k] = lds[0][at + dr[k % 3] + dc[k / 3]];
                w[k] = want_conf ? lds[1][at + dr[k % 3] + dc[k / 3]] : 0.0f;
            }
            slope_cell(g, w, dr[2] - dr[0], (c > 0 ? 1 : 0) + (c < cols - 1 ? 1 : 0), res, mask, v);
        }
        const size_t to = row_major ? (size_t)r * cols + (size_t)c : (size_t)r + (size_t)c * rows;
#pragma unroll
        for (int k = 0; k < GG_NUM_SLOPE_CHANNELS; ++k)
            if ((mask >> k) & 1u) plane[k][to] = v[k]; // (uniform)
    }
}

// Cell by cell in destination order: up to nine gathered pairs per cell.
__global__ __launch_bounds__(256) void k_slopes_gather(const Arena a, const PlaneArgs x)
{
    const ExportMap m = x.maps[blockIdx.y];
    const float2 *gp2 = gp2_ptr(a, m.slot);
    const int rows = a.g.rows, cols = a.g.cols;
    float *out = x.planes + (size_t)blockIdx.y * (size_t)x.n_planes * x.plane_stride;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const unsigned mask = x.mask;
    const float res = a.g.resolution_f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.g.C; i += gridDim.x * blockDim.x) {
        const int r = row_major ? i / cols : i % rows, c = row_major ? i % cols : i / rows;
        float v[GG_NUM_SLOPE_CHANNELS];
        if (m.fresh) { // (uniform)
            fresh_values(v);
        } else {
            const int rr[3] = {max(r - 1, 0), r, min(r + 1, rows - 1)};
            const int cc[3] = {max(c - 1, 0), c, min(c + 1, cols - 1)};
            float g[9], w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float2 p = gp2[gp_idx(a, rr[k % 3], cc[k / 3])];
                g[k] = p.x;
                w[k] = p.y;
            }
            slope_cell(g, w, rr[2] - rr[0], cc[2] - cc[0], res, mask, v);
        }
        int k = 0;
#pragma unroll
        for (int ch = 0; ch < GG_NUM_SLOPE_CHANNELS; ++ch) {
            if (!((mask >> ch) & 1u)) continue; // (uniform)
            out[(size_t)k * x.plane_stride + i] = v[ch];
            ++k;
        }
    }
}

void launch_slopes(const Arena &a, const PlaneArgs &x, int n_maps, int variant, hipStream_t s)
{
    for (int first = 0; first < n_maps; first += 32768) { // (gridDim.y, as launch_export)
        const int count = std::min(32768, n_maps - first);
        PlaneArgs part = x;
        part.maps = x.maps + first;
        part.planes = x.planes + (size_t)first * (size_t)x.n_planes * x.plane_stride;
        if (variant == 1)
            hipLaunchKernelGGL(k_slopes_gather, dim3(std::min((a.g.C + 255) / 256, n_maps >= 64 ? 64 : 2048), count), dim3(256), 0, s, a, part);
        else
            hipLaunchKernelGGL(k_slopes_tiled, dim3(x.blocks_r * x.blocks_c, count), dim3(256), 0, s, a, part);
    }
}

} // namespace gg
