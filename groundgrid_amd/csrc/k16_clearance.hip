// K16 -- gg_clearance_clouds: the exact OBSTACLE DISTANCE FIELD of MANY maps in device memory (include/groundgrid_hip.h): per cell the
// squared Euclidean distance, in cells, to the nearest occupied cell of the same map, which cell that is, and the distance in metres.  What a
// caller composes today from gg_cluster_clouds, a download, scipy.ndimage.distance_transform_edt per map on the host and an upload.
//
// The occupancy is that of gg_cluster_clouds (launch_cluster_occupancy, k15_cluster.hip: the same three launches on the same kind of plane)
// or a plane of the caller's (seed mode); occupied = the word is >= 0 as an int32 in either.  The d_dist2 plane is the only working memory
// (one 32-bit word per cell): the occupancy (cloud mode), then the signed row offset to the nearest occupied cell of the COLUMN, then dist2.
// Separable and exact, all in integers:
//   k_clearance_columns  one lane per column, down and up again: plane[r][c] := r' - r of the occupied cell (r', c) nearest to r in column c
//                        -- of two equally near ones the upper, r' < r -- or NONE.  The occupied cells of a column are counted on the way
//                        (one integer atomic add per wavefront into d_n_occupied)
//   k_clearance_rows     one work-group per row r: the row's offsets off[] go to LDS, and cell (r, c) minimises off[j]^2 + (c - j)^2 over j,
//                        equal sums ranked by (r + off[j], j), walking j outwards from c: j = c - d and c + d for d = 0, 1, ... while
//                        d^2 <= min(best so far, max_cells^2) -- a candidate d columns away is at least d^2 away.  The up to three outputs
//                        are written in place: a row is read and written by one work-group alone.
// The ranking is exact: of a column only the cells at the smallest vertical distance from r can attain the minimum over the map (any other
// cell of that column is strictly farther from (r, c)), they are at most two, and the first pass kept the one with the smaller row; so the
// second pass sees, per column, the smallest (distance, row) of that column, and its own order (distance, row, column) is the tie rule.
// No work-group waits for another, every loop is bounded by rows or cols, no float is added and the only atomic is an integer add: the
// outputs do not depend on scheduling.
//
// Algorithmic bytes: the occupancy as K15's (cloud mode: per input point 1 (labels; 0.25 with masks) + 16 (32: GG_POINT32), per participating
// point 8 gathered with a height band and one 4-byte atomic; per cell 4 written, 4 + 4 by the seed) or 4 read per cell (seed mode); per cell
// 4 written + 4 read + 4 written by the columns (cloud mode reads in place), 4 read + 4 written per given output by the rows.  Operations:
// per cell 2 steps of the column walk and, in the rows, 2 candidates (an LDS word, a multiply-add, a 64-bit compare) per step outwards, at
// most cols of them; a row without any offset is answered without a walk.
#include "cloud_walk.h"

namespace gg {

constexpr int32_t CLEARANCE_NONE = GG_CLEARANCE_NONE; // "no occupied cell": an offset between the passes, a dist2 at the end
constexpr uint32_t CLEARANCE_INF_BITS = 0x7F800000u;

// (map, item) of a work-group, grid (items, maps): a map's work-groups meet in one L2
GG_DEV void clearance_item(int &map, int &item)
{
    const uint32_t it = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    map = (int)(it / gridDim.x);
    item = (int)(it % gridDim.x);
}

// Cell (r, c) of a plane at r * sr + c * sc: (cols, 1) row-major, (1, rows) column-major.  Grid (ceil(cols / 64), maps), one wavefront each.
// With seeds == dist2 (cloud mode) a lane reads a word before it overwrites it, and nobody else touches its column.
__global__ __launch_bounds__(64) void k_clearance_columns(const Arena a, const ClearanceArgs x)
{
    int map, chunk;
    clearance_item(map, chunk);
    const int rows = a.g.rows, cols = a.g.cols;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const size_t sr = row_major ? (size_t)cols : 1, sc = row_major ? 1 : (size_t)rows;
    const int c = chunk * 64 + (int)threadIdx.x;
    uint32_t count = 0u;
    if (c < cols) {
        const int32_t *src = x.seeds + (size_t)map * x.seed_stride + (size_t)c * sc;
        int32_t *dst = x.dist2 + (size_t)map * x.plane_stride + (size_t)c * sc;
        int last = -1; // the nearest occupied row at or above r
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
            if (src[(size_t)r * sr] >= 0) {
                last = r;
                ++count;
            }
            dst[(size_t)r * sr] = last >= 0 ? last - r : CLEARANCE_NONE;
        }
        int next = -1; // the nearest occupied row at or below r
#pragma unroll 4
        for (int r = rows - 1; r >= 0; --r) {
            const int up = dst[(size_t)r * sr]; // <= 0, or NONE
            if (up == 0) next = r;
            else if (next >= 0 && (up == CLEARANCE_NONE || next - r < -up)) dst[(size_t)r * sr] = next - r; // (equally near: the upper stays)
        }
    }
    count = wave_sum(count); // (all 64 lanes are here)
    if (threadIdx.x == 0 && x.n_occupied && count) atomicAdd(reinterpret_cast<uint32_t *>(x.n_occupied) + map, count);
}

// Grid (rows, maps), min(1024, cols rounded up to 64) threads, cols words of dynamic LDS.
__global__ __launch_bounds__(1024) void k_clearance_rows(const Arena a, const ClearanceArgs x)
{
    extern __shared__ int32_t clearance_line[];
    int map, r;
    clearance_item(map, r);
    const int rows = a.g.rows, cols = a.g.cols;
    const bool row_major = x.order == GG_PLANES_ROWMAJOR;
    const size_t sc = row_major ? 1 : (size_t)rows;
    const size_t at = (size_t)map * x.plane_stride + (row_major ? (size_t)r * cols : (size_t)r);
    int32_t *dist2 = x.dist2 + at;
    bool mine = false;
    for (int c = (int)threadIdx.x; c < cols; c += (int)blockDim.x) {
        const int32_t o = dist2[(size_t)c * sc];
        clearance_line[c] = o;
        mine |= o != CLEARANCE_NONE;
    }
    const bool any = __syncthreads_or(mine) != 0; // (the only barrier; nothing below crosses lanes)
    int32_t *nearest = x.nearest ? x.nearest + at : nullptr;
    uint32_t *distance = x.distance ? reinterpret_cast<uint32_t *>(x.distance) + at : nullptr;
    const float res = a.g.resolution_f;
    for (int c = (int)threadIdx.x; c < cols; c += (int)blockDim.x) {
        uint64_t best = ~0ull;     // (dist2, row-major index of the cell): its order is (dist2, row, column)
        uint32_t bound = x.reach2; // a candidate above it cannot win
        if (any) {
            for (int d = 0; d <= x.reach && (uint32_t)(d * d) <= bound; ++d) { // (d <= cols: reach is)
                const int jl = c - d, jr = c + d;
                if (jl < 0 && jr >= cols) break;
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const int j = side ? jr : jl;
                    if (side ? (d == 0 || jr >= cols) : jl < 0) continue;
                    const int32_t o = clearance_line[j];
                    if (o == CLEARANCE_NONE) continue;
                    const uint32_t d2 = (uint32_t)(o * o + d * d);
                    const uint64_t key = ((uint64_t)d2 << 32) | (uint32_t)((r + o) * cols + j);
                    if (key < best) {
                        best = key;
                        bound = min(bound, d2);
                    }
                }
            }
        }
        const uint32_t d2 = (uint32_t)(best >> 32);
        const bool none = best == ~0ull || d2 > x.reach2;
        dist2[(size_t)c * sc] = none ? CLEARANCE_NONE : (int32_t)d2;
        if (nearest) {
            const int lin = (int)(uint32_t)best; // row-major
            nearest[(size_t)c * sc] = none ? -1 : row_major ? lin : lin / cols + (lin % cols) * rows;
        }
        if (distance) distance[(size_t)c * sc] = none ? CLEARANCE_INF_BITS : __float_as_uint(sqrtf((float)d2) * res);
    }
}

void launch_clearance(const Arena &a, const ClearanceArgs &x, int n_maps, hipStream_t s)
{
    if (x.from_clouds) launch_cluster_occupancy(a, x.occ, n_maps, s);
    if (x.n_occupied) (void)hipMemsetAsync(x.n_occupied, 0, sizeof(int32_t) * (size_t)n_maps, s);
    hipLaunchKernelGGL(k_clearance_columns, dim3((a.g.cols + 63) / 64, n_maps), dim3(64), 0, s, a, x);
    const int threads = min(1024, (a.g.cols + 63) / 64 * 64);
    hipLaunchKernelGGL(k_clearance_rows, dim3(a.g.rows, n_maps), dim3(threads), sizeof(int32_t) * (size_t)a.g.cols, s, a, x);
}

} // namespace gg
