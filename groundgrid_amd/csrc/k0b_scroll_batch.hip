// K0b -- GroundGrid::update (src/GroundGrid.cpp:83-147) for many maps in one set of launches (gg_move_maps).
//
// The scroll is a gather (scroll_core.h: new(i, j) = old((i + s0) mod n, (j + s1) mod n) or the exposed fill), so it cannot run in
// place without a grid-wide barrier.  Two passes per chunk of maps instead:
//   k_scroll_gather: one thread per cell of one map (grid.y = the chunk's maps) computes the cell's new value into a compact scratch row
//   k_scroll_commit: copies the scratch row back into the map's (ground, confidence) layer -- cell elements only, so that padding
//                    (the fresh padding element Arena::gp_fresh_cell among it) stays as it is.
// Cells are taken in the layer's element order (`cells`: the element and (row, col) of cell t, ascending elements, built once on the
// host): the scratch rows are written and read contiguously, the commit writes runs of consecutive elements, and the 64 cells of a wave
// mostly come from 64 consecutive rings of one wedge whose sources lie a near-constant distance away in the same wedge.
// Traffic per moved map: read the old cells, write and read the scratch row, write the new cells -- 4 x C x 8 bytes.
#include "scroll_core.h"

namespace gg {

__global__ __launch_bounds__(256) void k_scroll_gather(const Arena a, const int2 *__restrict__ cells, const MoveParams *__restrict__ mp,
                                                       float2 *__restrict__ scratch)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.g.C) return;
    const MoveParams &p = mp[blockIdx.y];
    const int rc = cells[t].y;
    scratch[(size_t)blockIdx.y * a.g.C + t] = scroll_value(a, gp2_ptr(a, p.slot), rc & 0xFFFF, rc >> 16, p.sp, p.fresh != 0, p.fresh_z);
}

__global__ __launch_bounds__(256) void k_scroll_commit(const Arena a, const int2 *__restrict__ cells, const MoveParams *__restrict__ mp,
                                                       const float2 *__restrict__ scratch)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.g.C) return;
    gp2_ptr(a, mp[blockIdx.y].slot)[cells[t].x] = scratch[(size_t)blockIdx.y * a.g.C + t];
}

// n_maps maps (d_params[0 .. n_maps)) through scratch rows [0, n_maps) of `scratch` (n_maps * C float2)
void launch_scroll_batch(const Arena &a, const int2 *cells, const MoveParams *d_params, int n_maps, float2 *scratch, hipStream_t s)
{
    const dim3 grid((a.g.C + 255) / 256, n_maps);
    hipLaunchKernelGGL(k_scroll_gather, grid, dim3(256), 0, s, a, cells, d_params, scratch);
    hipLaunchKernelGGL(k_scroll_commit, grid, dim3(256), 0, s, a, cells, d_params, (const float2 *)scratch);
}

} // namespace gg
