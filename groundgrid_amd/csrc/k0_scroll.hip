// K0 -- GroundGrid::update (src/GroundGrid.cpp:83-147) on the device: the map follows the vehicle.
//
// grid_map::GridMap::move shifts the map by a whole number of cells (the host computes the shift with grid_map's
// rounding, gg_context.hip gg_move_map), drops the rows / columns that fall out and exposes new ones;
// GroundGrid::update fills the exposed cells with ground = -(z of the cell centre expressed in base_link) and
// groundpatch = 0 (:121-131) and re-linearises the ring buffer (:143), which the hot path relies on (it indexes raw
// matrices).  In default-start-index terms that is one gather per cell:
//     new(i, j) = exposed(i, j) ? fill(i, j) : old((i + s0) mod n, (j + s1) mod n)
// Only `ground` and `groundpatch` persist across clouds (every other layer is rewritten by the next filter_cloud
// before anyone can observe it), so only those two are moved: 4 layer-passes per cloud instead of 22.
// The per-cell value is scroll_core.h scroll_value (shared with gg_move_maps, k0b_scroll_batch.hip).
#include "scroll_core.h"

namespace gg {

__global__ __launch_bounds__(256) void k_scroll(const Arena a, int slot, float2 *__restrict__ out, const ScrollParams sp)
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= a.g.rows || j >= a.g.cols) return;
    out[gp_idx(a, i, j)] = scroll_value(a, gp2_ptr(a, slot), i, j, sp, false, 0.0f); // same element order as the layer: copied back whole
}

void launch_scroll(const Arena &a, int slot, float2 *scratch, int s0, int s1, double pos_x, double pos_y, const double plane[4],
                   hipStream_t s)
{
    const ScrollParams sp = make_scroll_params(a, s0, s1, pos_x, pos_y, plane);
    dim3 grid((a.g.rows + 63) / 64, (a.g.cols + 3) / 4);
    hipLaunchKernelGGL(k_scroll, grid, dim3(256), 0, s, a, slot, scratch, sp);
    hipMemcpyAsync(gp2_ptr(a, slot), scratch, (size_t)a.gpl.elems * 8, hipMemcpyDeviceToDevice, s); // (elements no cell maps to are never read)
}

} // namespace gg
