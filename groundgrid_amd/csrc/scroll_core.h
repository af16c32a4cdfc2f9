// scroll_core.h -- the per-cell value of GroundGrid::update (src/GroundGrid.cpp:83-147), shared by the one-map scroll (k0_scroll.hip,
// gg_move_map) and the many-map scroll (k0b_scroll_batch.hip, gg_move_maps): both return bit for bit the same cells.
#pragma once

#include "gg_device.h"

namespace gg {

struct ScrollParams {
    int s0, s1;          // index shift (rows, cols), buffer order
    double pos_x, pos_y; // map position AFTER the move
    double first0, first1; // L/2 - res/2  (getVectorToFirstCell)
    double res;
    double m20, m21, m22, tz; // third row of the base_link<-map rotation and translation z (gg_move_map base_plane)
};

// one map of a gg_move_maps launch (the device array is indexed by blockIdx.y)
struct MoveParams {
    ScrollParams sp;
    int slot;
    int fresh;     // the map is FRESH (gg_context::fresh): every cell holds (fresh_z, 1e-7) by definition, none is read
    float fresh_z;
};

inline ScrollParams make_scroll_params(const Arena &a, int s0, int s1, double pos_x, double pos_y, const double plane[4])
{
    ScrollParams sp;
    sp.s0 = s0;
    sp.s1 = s1;
    sp.pos_x = pos_x;
    sp.pos_y = pos_y;
    sp.res = a.g.resolution;
    sp.first0 = a.g.half0 - 0.5 * a.g.resolution;
    sp.first1 = a.g.half1 - 0.5 * a.g.resolution;
    // third row of the base_link <- map rotation and translation z, as the binding built them (gg_move_map)
    sp.m20 = plane[0];
    sp.m21 = plane[1];
    sp.m22 = plane[2];
    sp.tz = plane[3];
    return sp;
}

// (ground, confidence) of cell (i, j) after the move:
//     new(i, j) = exposed(i, j) ? fill(i, j) : old((i + s0) mod n, (j + s1) mod n)
// `src` is the map's layer before the move; a fresh map's old cells are the reset's pair (fresh_z, 1e-7) and src is not read.
GG_DEV float2 scroll_value(const Arena &a, const float2 *src, int i, int j, const ScrollParams &sp, bool fresh, float fresh_z)
{
    const int rows = a.g.rows, cols = a.g.cols;
    const bool all = abs(sp.s0) >= rows || abs(sp.s1) >= cols;
    int bi = (i + sp.s0) % rows, bj = (j + sp.s1) % cols;
    if (bi < 0) bi += rows;
    if (bj < 0) bj += cols;
    const bool new0 = sp.s0 > 0 ? bi < sp.s0 : (sp.s0 < 0 ? bi >= rows + sp.s0 : false);
    const bool new1 = sp.s1 > 0 ? bj < sp.s1 : (sp.s1 < 0 ? bj >= cols + sp.s1 : false);
    if (all || new0 || new1) {
        // grid_map getPositionFromIndex: position = mapPosition + offset + resolution * (-index)
        const double px = (sp.pos_x + sp.first0) + sp.res * (double)(-i);
        const double py = (sp.pos_y + sp.first1) + sp.res * (double)(-j);
        // doTransform: v_out.z = (m20 * x + m21 * y + m22 * 0) + origin.z ; ground = -z (:130), groundpatch = 0 (:131)
        const double z = ((sp.m20 * px + sp.m21 * py) + sp.m22 * 0.0) + sp.tz;
        return make_float2((float)(-z), 0.0f);
    }
    if (fresh) return make_float2(fresh_z, (float)0.0000001); // (make_real's fill)
    return src[gp_idx(a, bi, bj)];
}

} // namespace gg
