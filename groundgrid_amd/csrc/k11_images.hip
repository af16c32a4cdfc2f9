// K11 -- gg_export_images: the 8-bit layer images and the 32FC3 terrain images of MANY maps in device memory (include/groundgrid_hip.h).
// What gg_get_layer_image_u8 and gg_get_terrain_image (k6_wire.hip) return per map and layer, without a dense float plane in between:
// the kernels read the layers where they are, with the walk of k9_export.hip -- one work-group per 64 x 64 block of cells of one map, the
// (ground, confidence) pairs in ELEMENT order through the export table, the per-call layers tile by tile behind their liveness words with
// the reset value for dead half columns, a fresh map's pair from the reset's constants --, and write bytes.
//
// u8 images, two launches (the normalisation needs the bounds of the whole plane first):
//   k_image_bounds_tiled   min / max over the finite cells of every named layer of its block, straight from the sources (no staging: a
//                          minimum does not care where a cell lies) -> one partial pair per (map, layer, block) in call scratch
//   k_image_u8_tiled       folds the partial pairs of its map (min and max do not depend on the order: the value k_minmax_finite gives),
//                          stages a layer's block in LDS (row + 65 * column) and writes the image's rows: four cells per lane as one 32-bit
//                          store wherever the destination word is whole, single bytes at the unaligned head and tail of a row's run --
//                          the destination needs no alignment and a byte outside the image is never touched.  Block 0 of a map also
//                          writes the bounds where the caller asked for them.
// terrain, one launch:
//   k_terrain_tiled        ground and pointsRaw of the block in LDS, pointsRaw with a one-cell halo (dead half columns and cells outside the
//                          map count 0), the flag "3 x 3 pointsRaw sum >= 27" in k_terrain_image's order (tree9, border cells 0) into a
//                          third block, then HWC rows as runs of 192 consecutive floats or CHW as three planes in runs of 64.
// gg_debug_set_tuning "images_variant" = 1 runs the call through the cell-by-cell forms below (the indexing of k_export_gather /
// k_terrain_image): the A/B of tools/bench_images.py and the tests' cross-check.
#include "gg_device.h"

#include <algorithm>

namespace gg {

constexpr int IMG_LD = EXPORT_TILE + 1;          // LDS pitch of a block: cell (row, col) at row + IMG_LD * col
constexpr int IMG_BLOCK = EXPORT_TILE * IMG_LD;  // floats of one staged block
constexpr int RAW_LD = EXPORT_TILE + 3;          // ... of the pointsRaw block with its halo: cell (row, col) at (row + 1) + RAW_LD * (col + 1), row / col -1 .. 64
constexpr int RAW_BLOCK = RAW_LD * (EXPORT_TILE + 2);
constexpr unsigned IMG_GP_MASK = (1u << GG_LAYER_GROUND) | (1u << GG_LAYER_GROUNDPATCH);

GG_DEV int image_plane_index(unsigned mask, int layer) { return __popc(mask & ((1u << layer) - 1u)); }

// min / max over finite values (k_minmax_finite's test and operations)
GG_DEV void mm_take(float &lo, float &hi, float v)
{
    if (isfinite(v)) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
}
GG_DEV void mm_wave(float &lo, float &hi)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    }
}

struct ImgBlock {
    int mt, mtr, mtc; // block, its block row and block column
    int r0, c0;       // first cell
    int nr, nc;       // cells of the block inside the map
};
GG_DEV ImgBlock img_block(const Arena &a, int blocks_r, int mt)
{
    ImgBlock b;
    b.mt = mt;
    b.mtr = mt % blocks_r;
    b.mtc = mt / blocks_r;
    b.r0 = b.mtr * EXPORT_TILE;
    b.c0 = b.mtc * EXPORT_TILE;
    b.nr = min(EXPORT_TILE, a.g.rows - b.r0);
    b.nc = min(EXPORT_TILE, a.g.cols - b.c0);
    return b;
}

// The per-call layers of a block: wavefront w owns tiles 4 w .. 4 w + 3 of the block's 4 x 4 tiles; a lane owns four consecutive rows of one
// column of a tile (16 bytes, half of one liveness bit's half column).
struct TileLanes {
    int rank[4];        // Morton rank of the tile, -1: the tile lies outside the map
    bool live[4];       // the lane's half column holds its values
    int ri[4], ci[4];   // the lane's first cell, in the block
    unsigned inside[4]; // bit q: row ri + q of column ci is a cell of the map
};
GG_DEV void tile_lanes(const Arena &a, const uint32_t *tile_live, const ImgBlock &b, int tid, TileLanes &t)
{
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = wave * 4 + j, ltr = k & 3, ltc = k >> 2;
        const int tr = b.mtr * (EXPORT_TILE / TILE) + ltr, tc = b.mtc * (EXPORT_TILE / TILE) + ltc;
        t.rank[j] = -1;
        t.live[j] = false;
        t.inside[j] = 0u;
        t.ri[j] = ltr * TILE + (lane & 3) * 4;
        t.ci[j] = ltc * TILE + (lane >> 2);
        if (tr < a.g.tiles_r && tc < a.g.tiles_c) {
            t.rank[j] = (int)a.tile_rank[tr + tc * a.g.tiles_r];
            t.live[j] = ((tile_live[t.rank[j]] >> live_bit(lane * 4)) & 1u) != 0u;
            if (t.ci[j] < b.nc)
                for (int q = 0; q < 4; ++q) t.inside[j] |= t.ri[j] + q < b.nr ? 1u << q : 0u;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- u8: the bounds launch

__global__ __launch_bounds__(256) void k_image_bounds_tiled(const Arena a, const ImageArgs x)
{
    __shared__ float s_lo[GG_NUM_LAYERS][4], s_hi[GG_NUM_LAYERS][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ExportMap m = x.maps[blockIdx.y];
    const ImgBlock b = img_block(a, x.blocks_r, (int)blockIdx.x);
    const float inf = __builtin_inff();
    auto put = [&](int layer, float lo, float hi) { // (uniform: every wavefront leaves its pair of plane k)
        mm_wave(lo, hi);
        if (lane == 0) {
            s_lo[image_plane_index(x.mask, layer)][wave] = lo;
            s_hi[image_plane_index(x.mask, layer)][wave] = hi;
        }
    };
    const unsigned gp_mask = x.mask & IMG_GP_MASK;
    if (gp_mask) {
        float lo0 = inf, hi0 = -inf, lo1 = inf, hi1 = -inf;
        if (m.fresh) { // the reset's values by definition: nothing of the layer is read
            mm_take(lo0, hi0, m.fresh_z);
            mm_take(lo1, hi1, (float)0.0000001);
        } else {
            const float2 *gp2 = gp2_ptr(a, m.slot);
            const uint32_t first = x.block_off[b.mt], end = x.block_off[b.mt + 1];
            for (uint32_t i = first + tid; i < end; i += 256) {
                const float2 v = gp2[x.elem[i]];
                mm_take(lo0, hi0, v.x);
                mm_take(lo1, hi1, v.y);
            }
        }
        if (gp_mask & (1u << GG_LAYER_GROUND)) put(GG_LAYER_GROUND, lo0, hi0);
        if (gp_mask & (1u << GG_LAYER_GROUNDPATCH)) put(GG_LAYER_GROUNDPATCH, lo1, hi1);
    }
    if (x.mask & ~gp_mask) { // (uniform)
        const float *percall = percall_ptr(a, m.slot);
        TileLanes t;
        tile_lanes(a, a.tile_live + (size_t)m.slot * a.tile_live_stride, b, tid, t);
        for (int l = 0; l < GG_NUM_LAYERS; ++l) {
            if (!((x.mask >> l) & 1u) || percall_position(l) < 0) continue; // (uniform)
            const float dead = layer_reset_value(l);
            const int position = percall_position(l);
            float lo = inf, hi = -inf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t.rank[j] < 0 || !t.inside[j]) continue;
                float4 v = make_float4(dead, dead, dead, dead);
                if (t.live[j]) v = *reinterpret_cast<const float4 *>(percall + percall_index(t.rank[j], position, lane * 4));
                if (t.inside[j] & 1u) mm_take(lo, hi, v.x);
                if (t.inside[j] & 2u) mm_take(lo, hi, v.y);
                if (t.inside[j] & 4u) mm_take(lo, hi, v.z);
                if (t.inside[j] & 8u) mm_take(lo, hi, v.w);
            }
            put(l, lo, hi);
        }
    }
    __syncthreads();
    if (tid < x.n_planes) {
        float lo = s_lo[tid][0], hi = s_hi[tid][0];
        for (int w = 1; w < 4; ++w) {
            lo = fminf(lo, s_lo[tid][w]);
            hi = fmaxf(hi, s_hi[tid][w]);
        }
        float *part = x.partials + (((size_t)blockIdx.y * x.n_planes + tid) * x.n_parts + b.mt) * 2;
        part[0] = lo;
        part[1] = hi;
    }
}

// the bounds of every plane of map `map` from the partial pairs of the bounds launch -> s_b[k] = (lower, upper); ends in a barrier
GG_DEV void fold_bounds(const ImageArgs &x, int map, float (*s_b)[2], int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < x.n_planes; k += 4) {
        const float *p = x.partials + ((size_t)map * x.n_planes + k) * x.n_parts * 2;
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int q = lane; q < x.n_parts; q += 64) {
            lo = fminf(lo, p[2 * q]);
            hi = fmaxf(hi, p[2 * q + 1]);
        }
        mm_wave(lo, hi);
        if (lane == 0) {
            s_b[k][0] = lo;
            s_b[k][1] = hi;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- u8: the image launch

// One staged block -> the rows of its image.  The run of row ri is nc bytes from img + (r0 + ri) * cols + c0; it is cut at the 32-bit words of
// the DESTINATION ADDRESS (up to 17 touch a run of 64 bytes): a word that lies wholly inside the run is one store of four cells, the words
// at the run's head and tail give their bytes inside the run one by one.  Nothing outside the run is read or written.
GG_DEV void store_u8_block(uint8_t *img, const float *blk, const ImgBlock &b, int cols, float lo, float hi, int tid)
{
    constexpr int WORDS = EXPORT_TILE / 4 + 1;
    for (int idx = tid; idx < EXPORT_TILE * WORDS; idx += 256) {
        const int ri = idx / WORDS, w = idx - ri * WORDS;
        if (ri >= b.nr) break;
        uint8_t *row = img + (size_t)(b.r0 + ri) * cols + (size_t)b.c0;
        const int c = 4 * w - (int)(reinterpret_cast<uintptr_t>(row) & 3u); // first cell of the word (a column of the block; negative: in front of the run)
        if (c >= b.nc) continue;
        if (c >= 0 && c + 4 <= b.nc) {
            uint32_t v = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (uint32_t)layer_value_to_u8(blk[ri + (c + q) * IMG_LD], lo, hi) << (8 * q);
            *reinterpret_cast<uint32_t *>(row + c) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c + q >= 0 && c + q < b.nc) row[c + q] = layer_value_to_u8(blk[ri + (c + q) * IMG_LD], lo, hi);
        }
    }
}

__global__ __launch_bounds__(256) void k_image_u8_tiled(const Arena a, const ImageArgs x)
{
    __shared__ float lds[2][IMG_BLOCK];
    __shared__ float s_b[GG_NUM_LAYERS][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const ExportMap m = x.maps[blockIdx.y];
    const ImgBlock b = img_block(a, x.blocks_r, (int)blockIdx.x);
    const int cols = a.g.cols;
    fold_bounds(x, (int)blockIdx.y, s_b, tid);
    if (b.mt == 0 && x.bounds && tid < 2 * x.n_planes) x.bounds[(size_t)blockIdx.y * x.n_planes * 2 + tid] = s_b[tid >> 1][tid & 1];
    uint8_t *out = x.images + (size_t)blockIdx.y * (size_t)x.n_planes * x.image_stride;
    auto store = [&](int layer, const float *blk) {
        const int k = image_plane_index(x.mask, layer);
        store_u8_block(out + (size_t)k * x.image_stride, blk, b, cols, s_b[k][0], s_b[k][1], tid);
    };

    const unsigned gp_mask = x.mask & IMG_GP_MASK;
    if (gp_mask) {
        if (m.fresh) { // the reset's values by definition (gg_context::fresh): nothing of the layer is read
            const float z = m.fresh_z, w = (float)0.0000001;
            for (int i = tid; i < IMG_BLOCK; i += 256) {
                lds[0][i] = z;
                lds[1][i] = w;
            }
        } else {
            const float2 *gp2 = gp2_ptr(a, m.slot);
            const uint32_t first = x.block_off[b.mt], end = x.block_off[b.mt + 1];
            for (uint32_t i = first + tid; i < end; i += 256) {
                const float2 v = gp2[x.elem[i]];
                const uint32_t c = x.cell[i]; // row in block | column in block << 6
                const int at = (int)(c & 63u) + (int)(c >> 6) * IMG_LD;
                lds[0][at] = v.x;
                lds[1][at] = v.y;
            }
        }
        __syncthreads();
        if (gp_mask & (1u << GG_LAYER_GROUND)) store(GG_LAYER_GROUND, lds[0]);
        if (gp_mask & (1u << GG_LAYER_GROUNDPATCH)) store(GG_LAYER_GROUNDPATCH, lds[1]);
    }
    if (!(x.mask & ~gp_mask)) return; // (uniform)

    const float *percall = percall_ptr(a, m.slot);
    TileLanes t;
    tile_lanes(a, a.tile_live + (size_t)m.slot * a.tile_live_stride, b, tid, t);
    __syncthreads(); // (the stores of the pairs above have read both LDS blocks)
    int buf = 0;     // the two blocks alternate: a layer's staging never meets the stores of the layer before it, one barrier per layer
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!((x.mask >> l) & 1u) || percall_position(l) < 0) continue; // (uniform)
        const float dead = layer_reset_value(l);
        const int position = percall_position(l);
        float *blk = lds[buf];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (t.rank[j] < 0) continue;
            float4 v = make_float4(dead, dead, dead, dead);
            if (t.live[j]) v = *reinterpret_cast<const float4 *>(percall + percall_index(t.rank[j], position, lane * 4));
            const int at = t.ri[j] + t.ci[j] * IMG_LD;
            blk[at + 0] = v.x;
            blk[at + 1] = v.y;
            blk[at + 2] = v.z;
            blk[at + 3] = v.w;
        }
        __syncthreads();
        store(l, blk);
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- terrain

__global__ __launch_bounds__(256) void k_terrain_tiled(const Arena a, const ImageArgs x)
{
    __shared__ float lds[2 * IMG_BLOCK + RAW_BLOCK];
    float *s_ground = lds, *s_flag = lds + IMG_BLOCK, *s_raw = lds + 2 * IMG_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63;
    const ExportMap m = x.maps[blockIdx.y];
    const ImgBlock b = img_block(a, x.blocks_r, (int)blockIdx.x);
    const int rows = a.g.rows, cols = a.g.cols;

    // channel 0: ground (the pair's first half, in element order; a fresh map: the reset's height)
    if (m.fresh) {
        for (int i = tid; i < IMG_BLOCK; i += 256) s_ground[i] = m.fresh_z;
    } else {
        const float *gpf = reinterpret_cast<const float *>(gp2_ptr(a, m.slot));
        const uint32_t first = x.block_off[b.mt], end = x.block_off[b.mt + 1];
        for (uint32_t i = first + tid; i < end; i += 256) {
            const uint32_t c = x.cell[i];
            s_ground[(int)(c & 63u) + (int)(c >> 6) * IMG_LD] = gpf[(size_t)x.elem[i] * 2];
        }
    }
    // channel 2: pointsRaw of the block tile by tile (0 in dead half columns and in tiles outside the map) ...
    const float *percall = percall_ptr(a, m.slot);
    TileLanes t;
    tile_lanes(a, a.tile_live + (size_t)m.slot * a.tile_live_stride, b, tid, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t.rank[j] >= 0 && t.live[j]) v = *reinterpret_cast<const float4 *>(percall + percall_index(t.rank[j], PL_POINTSRAW, lane * 4));
        const int at = (t.ri[j] + 1) + (t.ci[j] + 1) * RAW_LD;
        s_raw[at + 0] = v.x;
        s_raw[at + 1] = v.y;
        s_raw[at + 2] = v.z;
        s_raw[at + 3] = v.w;
    }
    // ... and its one-cell halo cell by cell: the rows above and below (66 cells each, corners included), the columns left and right (64 each)
    for (int h = tid; h < 4 * EXPORT_TILE + 4; h += 256) {
        int ri, ci;
        if (h < EXPORT_TILE + 2) {
            ri = -1;
            ci = h - 1;
        } else if (h < 2 * (EXPORT_TILE + 2)) {
            ri = EXPORT_TILE;
            ci = h - (EXPORT_TILE + 2) - 1;
        } else if (h < 2 * (EXPORT_TILE + 2) + EXPORT_TILE) {
            ri = h - 2 * (EXPORT_TILE + 2);
            ci = -1;
        } else {
            ri = h - 2 * (EXPORT_TILE + 2) - EXPORT_TILE;
            ci = EXPORT_TILE;
        }
        const int r = b.r0 + ri, c = b.c0 + ci;
        float v = 0.0f;
        if (r >= 0 && c >= 0 && r < rows && c < cols && cell_is_live(a, m.slot, r, c)) v = percall[percall_index_of(a, PL_POINTSRAW, r, c)];
        s_raw[(ri + 1) + (ci + 1) * RAW_LD] = v;
    }
    __syncthreads();
    // channel 1: Nodelet.cpp:258-268 as k_terrain_image has it -- the 3 x 3 block in column-major order through tree9, border cells of the MAP 0
    for (int idx = tid; idx < EXPORT_TILE * EXPORT_TILE; idx += 256) {
        const int ri = idx & (EXPORT_TILE - 1), ci = idx >> 6;
        if (ri >= b.nr || ci >= b.nc) continue;
        const int i = b.r0 + ri, j = b.c0 + ci;
        float flag = 0.0f;
        if (i >= 1 && j >= 1 && i + 1 < rows && j + 1 < cols) {
            float e[9];
#pragma unroll
            for (int s = 0; s < 9; ++s) e[s] = s_raw[(ri + s % 3) + (ci + s / 3) * RAW_LD]; // cell (ri - 1 + s % 3, ci - 1 + s / 3)
            flag = tree9(e) >= 27.0f ? 1.0f : 0.0f;
        }
        s_flag[ri + ci * IMG_LD] = flag;
    }
    __syncthreads();
    float *out = x.terrain + (size_t)blockIdx.y * x.terrain_stride;
    auto channel_at = [&](int ch, int ri, int ci) { return ch == 2 ? 2 * IMG_BLOCK + (ri + 1) + (ci + 1) * RAW_LD : ch * IMG_BLOCK + ri + ci * IMG_LD; };
    if (x.terrain_layout == GG_TERRAIN_HWC) { // a block row is 3 nc consecutive floats of the image: a wavefront store covers 64 of them
        for (int idx = tid; idx < EXPORT_TILE * EXPORT_TILE * 3; idx += 256) {
            const int ri = idx / (EXPORT_TILE * 3), f = idx - ri * (EXPORT_TILE * 3), ci = f / 3, ch = f - ci * 3;
            if (ri >= b.nr) break;
            if (ci >= b.nc) continue;
            out[((size_t)(b.r0 + ri) * cols + (size_t)b.c0) * 3 + f] = lds[channel_at(ch, ri, ci)];
        }
    } else { // three row-major planes, runs of 64 floats
        for (int ch = 0; ch < 3; ++ch)
            for (int idx = tid; idx < EXPORT_TILE * EXPORT_TILE; idx += 256) {
                const int ci = idx & (EXPORT_TILE - 1), ri = idx >> 6;
                if (ri >= b.nr || ci >= b.nc) continue;
                out[(size_t)ch * a.g.C + (size_t)(b.r0 + ri) * cols + (size_t)(b.c0 + ci)] = lds[channel_at(ch, ri, ci)];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- variant 1: cell by cell

// the value of every layer of cell (r, c) the mask names, as k_export_gather works it out; f(layer, value) in gg_layer order
template <class F> GG_DEV void cell_layers(const Arena &a, const ExportMap &m, unsigned mask, int r, int c, F f)
{
    const bool any_percall = (mask & ~IMG_GP_MASK) != 0u;
    const float *src = percall_ptr(a, m.slot);
    bool live = false;
    size_t at = 0;
    if (any_percall) {
        live = cell_is_live(a, m.slot, r, c);
        at = percall_index_of(a, 0, r, c);
    }
    float2 g = make_float2(m.fresh_z, (float)0.0000001);
    if (!m.fresh && (mask & IMG_GP_MASK)) g = gp2_ptr(a, m.slot)[gp_idx(a, r, c)];
#pragma unroll
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!((mask >> l) & 1u)) continue; // (uniform)
        float v;
        if (l == GG_LAYER_GROUND) v = g.x;
        else if (l == GG_LAYER_GROUNDPATCH) v = g.y;
        else v = live ? src[at + (size_t)percall_position(l) * (TILE * TILE)] : layer_reset_value(l);
        f(l, v);
    }
}

__global__ __launch_bounds__(256) void k_image_bounds_gather(const Arena a, const ImageArgs x)
{
    __shared__ float s_lo[GG_NUM_LAYERS][4], s_hi[GG_NUM_LAYERS][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ExportMap m = x.maps[blockIdx.y];
    const int cols = a.g.cols;
    float lo[GG_NUM_LAYERS], hi[GG_NUM_LAYERS];
#pragma unroll
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        lo[l] = __builtin_inff();
        hi[l] = -__builtin_inff();
    }
    for (int i = blockIdx.x * 256 + tid; i < a.g.C; i += gridDim.x * 256) cell_layers(a, m, x.mask, i / cols, i % cols, [&](int l, float v) { mm_take(lo[l], hi[l], v); });
#pragma unroll
    for (int l = 0; l < GG_NUM_LAYERS; ++l) {
        if (!((x.mask >> l) & 1u)) continue; // (uniform)
        mm_wave(lo[l], hi[l]);
        if (lane == 0) {
            s_lo[image_plane_index(x.mask, l)][wave] = lo[l];
            s_hi[image_plane_index(x.mask, l)][wave] = hi[l];
        }
    }
    __syncthreads();
    if (tid < x.n_planes) {
        float l0 = s_lo[tid][0], h0 = s_hi[tid][0];
        for (int w = 1; w < 4; ++w) {
            l0 = fminf(l0, s_lo[tid][w]);
            h0 = fmaxf(h0, s_hi[tid][w]);
        }
        float *part = x.partials + (((size_t)blockIdx.y * x.n_planes + tid) * x.n_parts + blockIdx.x) * 2;
        part[0] = l0;
        part[1] = h0;
    }
}

__global__ __launch_bounds__(256) void k_image_u8_gather(const Arena a, const ImageArgs x)
{
    __shared__ float s_b[GG_NUM_LAYERS][2];
    const int tid = threadIdx.x;
    const ExportMap m = x.maps[blockIdx.y];
    const int cols = a.g.cols;
    fold_bounds(x, (int)blockIdx.y, s_b, tid);
    if (blockIdx.x == 0 && x.bounds && tid < 2 * x.n_planes) x.bounds[(size_t)blockIdx.y * x.n_planes * 2 + tid] = s_b[tid >> 1][tid & 1];
    uint8_t *out = x.images + (size_t)blockIdx.y * (size_t)x.n_planes * x.image_stride;
    for (int i = blockIdx.x * 256 + tid; i < a.g.C; i += gridDim.x * 256)
        cell_layers(a, m, x.mask, i / cols, i % cols, [&](int l, float v) {
            const int k = image_plane_index(x.mask, l);
            out[(size_t)k * x.image_stride + i] = layer_value_to_u8(v, s_b[k][0], s_b[k][1]);
        });
}

// k_terrain_image for the listed maps, either layout; a fresh map's ground is the reset's height
__global__ __launch_bounds__(256) void k_terrain_gather(const Arena a, const ImageArgs x)
{
    const ExportMap m = x.maps[blockIdx.y];
    const float2 *gp2 = gp2_ptr(a, m.slot);
    const float *percall = percall_ptr(a, m.slot);
    const int rows = a.g.rows, cols = a.g.cols;
    float *out = x.terrain + (size_t)blockIdx.y * x.terrain_stride;
    auto raw_at = [&](int r, int c) { return cell_is_live(a, m.slot, r, c) ? percall[percall_index_of(a, PL_POINTSRAW, r, c)] : 0.0f; };
    for (int k = blockIdx.x * 256 + threadIdx.x; k < a.g.C; k += gridDim.x * 256) {
        const int i = k / cols, j = k % cols;
        float flag = 0.0f;
        if (i >= 1 && j >= 1 && i + 1 < rows && j + 1 < cols) {
            float e[9];
#pragma unroll
            for (int s = 0; s < 9; ++s) e[s] = raw_at(i - 1 + s % 3, j - 1 + s / 3);
            flag = tree9(e) >= 27.0f ? 1.0f : 0.0f;
        }
        const float ground = m.fresh ? m.fresh_z : gp2[gp_idx(a, i, j)].x;
        const bool hwc = x.terrain_layout == GG_TERRAIN_HWC;
        const size_t step = hwc ? (size_t)1 : (size_t)a.g.C;
        float *px = out + (hwc ? (size_t)k * 3 : (size_t)k);
        px[0] = ground;
        px[step] = flag;
        px[2 * step] = raw_at(i, j);
    }
}

void launch_images(const Arena &a, const ImageArgs &x, int n_maps, int variant, hipStream_t s)
{
    for (int first = 0; first < n_maps; first += 32768) { // (gridDim.y: one set of launches for every context of up to 32768 maps)
        const int count = std::min(32768, n_maps - first);
        ImageArgs part = x;
        part.maps = x.maps + first;
        if (x.images) part.images = x.images + (size_t)first * (size_t)x.n_planes * x.image_stride;
        if (x.partials) part.partials = x.partials + (size_t)first * (size_t)x.n_planes * (size_t)x.n_parts * 2;
        if (x.bounds) part.bounds = x.bounds + (size_t)first * (size_t)x.n_planes * 2;
        if (x.terrain) part.terrain = x.terrain + (size_t)first * x.terrain_stride;
        const dim3 tiled(x.blocks_r * x.blocks_c, count), gather(image_parts(a.g, 1), count);
        if (x.mask) { // (the bounds launch writes x.n_parts partial pairs per plane: the image launch folds exactly those)
            if (variant == 1) {
                hipLaunchKernelGGL(k_image_bounds_gather, gather, dim3(256), 0, s, a, part);
                hipLaunchKernelGGL(k_image_u8_gather, gather, dim3(256), 0, s, a, part);
            } else {
                hipLaunchKernelGGL(k_image_bounds_tiled, tiled, dim3(256), 0, s, a, part);
                hipLaunchKernelGGL(k_image_u8_tiled, tiled, dim3(256), 0, s, a, part);
            }
        }
        if (x.terrain) {
            if (variant == 1)
                hipLaunchKernelGGL(k_terrain_gather, gather, dim3(256), 0, s, a, part);
            else
                hipLaunchKernelGGL(k_terrain_tiled, tiled, dim3(256), 0, s, a, part);
        }
    }
}

} // namespace gg
