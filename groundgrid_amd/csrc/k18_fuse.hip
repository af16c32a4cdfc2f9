// K18 -- gg_fuse_states: the occupancy grid that PERSISTS ACROSS SCANS, for MANY maps in device memory (include/groundgrid_hip.h): the integer
// evidence of every cell scrolled by the map's index shift, decayed, moved by this scan's observation (a d_state plane of
// gg_visibility_clouds as it stands) and clamped; the three-valued state the evidence gives; and the exploration frontier, the free cells
// with an unknown neighbour.  What a caller composes today in torch from a shifted copy into a zeroed buffer, where, clamp and two
// thresholds, and an eight-neighbour max-pool: several full passes over every plane.
//
// One launch, grid (tiles, maps), 256 threads.  A plane is `ny` lines of `nx` contiguous words (row-major: nx = cols; column-major: nx =
// rows; the eight-neighbourhood is its own transpose, so one kernel serves both orders on (x, y) with the shift's components swapped).  A
// work-group owns a tile of FUSE_TILE_X x FUSE_TILE_Y = 62 x 26 cells and computes E and F on the 64 x 28 region around it, the tile plus a
// one-cell halo: lane l of a wavefront is column x0 - 1 + l of the region, wavefront w takes lines w, w + 4, ... (seven each).  So a line
// of the region is one wavefront's 64 consecutive dwords of d_state and of the shifted d_evidence_in (dword loads: the shifted address is
// in general not 16-byte aligned, and the lanes coalesce either way), all fourteen loads of a thread are issued before the first use, and
// the halo is recomputed from memory, never exchanged: no work-group waits for another.
// The frontier needs no plane of F in LDS.  A line's UNKNOWN cells are one 64-bit ballot u of the wavefront that holds it; h = u | u << 1 |
// u >> 1 is "this column or a side neighbour is unknown", and the 28 words h[line] are all the LDS the stencil takes.  After one barrier
// cell (line, lane) is a frontier iff F == FREE and bit `lane` of h[line - 1] | h[line] | h[line + 1] is set (the cell itself is FREE, so
// its own bit of h[line] is a neighbour's).  Cells of the region beyond the map's border are not UNKNOWN: they are no neighbours.
// E, F and the frontier are written for the tile's cells inside the map only, each output under a uniform branch; the words between
// rows * cols and a stride are never addressed.  Counts: per thread, summed over the lanes, then over the four wavefronts through LDS, and
// at most four integer atomic adds per work-group (k_visibility_states measured what one set per wavefront costs).
//
// Integers only.  |P|, |D| <= 2^30 - 1 and hit, miss, decay <= 2^30 - 1 (the entry point checks), so P -+ decay and D +- hit / miss stay inside
// an int32.  The shift reaches the kernel clamped to [-rows, rows] x [-cols, cols], which the definition makes equivalent (from |s| = side on
// no prior lies inside the map) and which keeps x + sx inside an int32.
//
// Algorithmic bytes per cell: 4 read (state) + 4 read (evidence in; none when NULL or exposed) + 4 written per given output (evidence,
// fused, frontier): 20 with everything.  The halo re-reads (64 * 28) / (62 * 26) = 1.11 of the inputs, mostly from L2: the tiles of a map
// run on one XCD (xcd_contiguous_item).  The tile is as wide as a wavefront minus the halo, so every load is one full-wavefront request; it
// is 26 lines tall because 28 lines are seven per wavefront (registers: seven E and F each), which keeps the re-read at 8 % along y.
#include "gg_device.h"

namespace gg {

constexpr int FUSE_LINES = FUSE_TILE_Y + 2;      // lines of a work-group's region
constexpr int FUSE_PER_WAVE = FUSE_LINES / 4;    // ... of one wavefront
static_assert(FUSE_TILE_X == 62, "a line of the region is one wavefront");
static_assert(FUSE_LINES % 4 == 0, "the region's lines split evenly over four wavefronts");

GG_DEV uint32_t fuse_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_fuse_states(const FuseArgs x)
{
    __shared__ unsigned long long unknown_near[FUSE_LINES]; // h of every line of the region
    __shared__ uint32_t wave_counts[4][3];
    const uint32_t it = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int map = (int)(it / gridDim.x), tile = (int)(it % gridDim.x);
    const int nx = x.nx, ny = x.ny;
    const int x0 = (tile % x.tiles_x) * FUSE_TILE_X, y0 = (tile / x.tiles_x) * FUSE_TILE_Y;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int2 sh = x.shifts ? x.shifts[map] : make_int2(0, 0); // (sx, sy), clamped by the entry point
    const int32_t *state = x.state + (size_t)map * x.state_stride;
    const int32_t *prior = x.evidence_in ? x.evidence_in + (size_t)map * x.plane_stride : nullptr;
    const size_t out = (size_t)map * x.plane_stride;

    const int gx = x0 - 1 + lane, px = gx + sh.x;
    const bool x_in = gx >= 0 && gx < nx, px_in = px >= 0 && px < nx;
    int32_t s[FUSE_PER_WAVE], p[FUSE_PER_WAVE];
#pragma unroll
    for (int j = 0; j < FUSE_PER_WAVE; ++j) {
        const int gy = y0 - 1 + wave + 4 * j, py = gy + sh.y;
        const bool in_map = x_in && gy >= 0 && gy < ny;
        s[j] = in_map ? state[gy * nx + gx] : 0;
        p[j] = in_map && prior && px_in && py >= 0 && py < ny ? prior[py * nx + px] : 0;
    }
    int32_t E[FUSE_PER_WAVE], F[FUSE_PER_WAVE];
#pragma unroll
    for (int j = 0; j < FUSE_PER_WAVE; ++j) {
        const int line = wave + 4 * j, gy = y0 - 1 + line;
        const bool in_map = x_in && gy >= 0 && gy < ny;
        const int32_t P = min(max(p[j], x.e_min), x.e_max);
        const int32_t D = P > 0 ? max(P - x.decay, 0) : min(P + x.decay, 0);
        E[j] = min(max(D + (s[j] > 0 ? x.hit : s[j] < 0 ? -x.miss : 0), x.e_min), x.e_max);
        F[j] = E[j] >= x.occ_threshold ? GG_CELL_OCCUPIED : E[j] <= x.free_threshold ? GG_CELL_FREE : GG_CELL_UNKNOWN;
        const unsigned long long u = __ballot(in_map && F[j] == GG_CELL_UNKNOWN); // (all 64 lanes are here)
        if (lane == 0) unknown_near[line] = u | (u << 1) | (u >> 1);
    }
    __syncthreads();
    uint32_t n_free = 0u, n_occupied = 0u, n_frontier = 0u;
    const bool x_own = lane >= 1 && lane <= FUSE_TILE_X && gx < nx; // (gx >= 0: lane >= 1)
#pragma unroll
    for (int j = 0; j < FUSE_PER_WAVE; ++j) {
        const int line = wave + 4 * j, gy = y0 - 1 + line;
        if (!(x_own && line >= 1 && line <= FUSE_TILE_Y && gy < ny)) continue; // (no cross-lane operation below)
        const unsigned long long near = unknown_near[line - 1] | unknown_near[line] | unknown_near[line + 1];
        const bool frontier = F[j] == GG_CELL_FREE && ((near >> lane) & 1ull) != 0ull;
        const size_t cell = out + (size_t)(gy * nx + gx);
        x.evidence_out[cell] = E[j];
        if (x.fused) x.fused[cell] = F[j];
        if (x.frontier) x.frontier[cell] = frontier ? 0 : -1;
        n_free += F[j] == GG_CELL_FREE;
        n_occupied += F[j] == GG_CELL_OCCUPIED;
        n_frontier += frontier;
    }
    if (!x.counts) return; // (uniform)
    n_free = fuse_wave_sum(n_free); // (every lane is back here)
    n_occupied = fuse_wave_sum(n_occupied);
    n_frontier = fuse_wave_sum(n_frontier);
    if (lane == 0) {
        wave_counts[wave][0] = n_free;
        wave_counts[wave][1] = n_occupied;
        wave_counts[wave][2] = n_frontier;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n_f = (int)(wave_counts[0][0] + wave_counts[1][0] + wave_counts[2][0] + wave_counts[3][0]);
    const int n_o = (int)(wave_counts[0][1] + wave_counts[1][1] + wave_counts[2][1] + wave_counts[3][1]);
    const int n_fr = (int)(wave_counts[0][2] + wave_counts[1][2] + wave_counts[2][2] + wave_counts[3][2]);
    const int n_u = (min(x0 + FUSE_TILE_X, nx) - x0) * (min(y0 + FUSE_TILE_Y, ny) - y0) - n_f - n_o;
    int32_t *counts = x.counts + (size_t)map * 4; // free, unknown, occupied, frontier
    if (n_f) atomicAdd(counts + 0, n_f);
    if (n_u) atomicAdd(counts + 1, n_u);
    if (n_o) atomicAdd(counts + 2, n_o);
    if (n_fr) atomicAdd(counts + 3, n_fr);
}

void launch_fuse(const FuseArgs &x, int n_maps, hipStream_t s)
{
    if (x.counts) (void)hipMemsetAsync(x.counts, 0, sizeof(int32_t) * 4 * (size_t)n_maps, s);
    const int tiles_y = (x.ny + FUSE_TILE_Y - 1) / FUSE_TILE_Y;
    hipLaunchKernelGGL(k_fuse_states, dim3(x.tiles_x * tiles_y, n_maps), dim3(256), 0, s, x);
}

} // namespace gg
