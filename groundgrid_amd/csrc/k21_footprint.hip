// K21 -- gg_footprint_planes: WHICH HEADINGS A VEHICLE FOOTPRINT FITS, per cell, for MANY maps in device memory (include/groundgrid_hip.h): for
// every cell and each of K <= 32 headings, whether the heading's cell set F_k -- a span (lo, hi) per row offset a in [-R, R], R <= 32 -- laid
// over the map at that cell touches a blocked cell.  What a caller composes today from K dense correlations with kernels of up to 65 x 65
// per map: K |F| look-ups per cell.  Here the test is bit-parallel over a line: 64 cells and one row of one heading are two shifts and three
// ANDs of 64-bit words.
//
// One launch, grid (tiles, maps), 256 threads.  A plane is `ny` lines of `nx` contiguous words (row-major: nx = cols; column-major: nx = rows,
// and the entry point hands over the transposed span table, which column-convexity makes exact: the kernel knows lines and positions along
// a line alone).  A work-group owns a tile of 64 x 64 cells at (x0, y0) and works in three phases with two barriers between them.
//   bitmap   The region is the 64 + 2 R lines y0 - R .. y0 + 63 + R and the 128 positions x0 - 32 .. x0 + 95 of each.  Wavefront w takes lines
//            w, w + 4, ...; a line is two loads of 64 consecutive words (lanes beyond x0 - R .. x0 + 63 + R repeat its last word) and two ballots of
//            "blocked": word >= 0 inside the map, the outside rule beyond it.  The complement F is the line's 128-bit word of FREE cells,
//            bit i = position x0 - 32 + i.  Its erosions E_p[i] = F[i] & ... & F[i + p - 1] for p = 1, 2, 4, ... follow by log steps
//            (E_2p = E_p & E_p >> p; the values are uniform over the wavefront) and go to LDS, one 16-byte word per line and level: at most
//            7 levels x 128 lines x 16 B = 14 KiB.  The halo is re-read from memory (mostly the L2 of the XCD the tiles of a map share:
//            xcd_contiguous_item), never exchanged: no work-group waits for another.
//   fits     Wavefront w takes the headings w, w + 4, ...; lane l is line y0 + l of the tile.  For every non-empty row j of the heading
//            (the packed table word is uniform: a scalar load) the lane reads E_p of line l + j, p the largest power of two <= the span's
//            width w, with one 16-byte LDS read (consecutive lanes, consecutive 16 bytes), and takes the 64 bits from bit lo + 32 and from
//            bit lo + 32 + w - p: their AND is "the w cells from x + lo on are free" for the 64 cells x of the tile's line.  The AND over
//            the rows is "heading k fits" for those 64 cells, one 64-bit word per (k, line) in LDS (16 KiB).
//   gather   Wavefront w takes the lines w, w + 4, ... of the tile, lane l is cell x0 + l: it collects its bit from the K words of its line
//            (LDS broadcast reads), and stores the mask and the fit word coalesced, each under a uniform branch, for the cells inside the
//            map alone; the words between rows * cols and a stride are never addressed.  Counts: per thread, summed over the lanes, then
//            over the four wavefronts through LDS, and at most three integer atomic adds per work-group, as k_fuse_states.
//
// Loop bounds: lines of the region <= 128 (32 per wavefront, in batches of 8 whose 16 loads are issued before the first ballot), levels <= 7,
// headings <= 32, rows <= 65, lines of the tile 64: all static.  Bits: a row reads bit positions i + lo + 32 .. i + hi + 32 of a line's word
// for 0 <= i <= 63, so 0 .. 127 by |lo|, |hi| <= 32 (the entry point checks): the zeros a shift brings in from beyond bit 127 are never
// looked at.  Indices: gy * nx + gx < rows * cols < 2^31.
//
// Algorithmic bytes per cell: 4 read + 4 written per given plane.  The region re-reads (64 + 2 R) (64 + 2 R) / 64^2 of the input, 2.1 times
// at R = 14, from L2.  Work per tile: K (2 R + 1) wavefront steps of one LDS read and about a dozen 64-bit operations, against 4096 cells.
#include "gg_device.h"

namespace gg {

constexpr int FOOTPRINT_LINES = FOOTPRINT_TILE + 2 * FOOTPRINT_MAX_RADIUS; // the most lines of its region
constexpr int FOOTPRINT_LEVELS = 7;                                      // erosions by 1, 2, ..., 64: a span is at most 65 wide
constexpr int FOOTPRINT_BATCH = 8;                                       // lines a wavefront loads before its first ballot
static_assert(FOOTPRINT_TILE == 64 && FOOTPRINT_MAX_RADIUS == 32, "a line of the region is two ballots: 32 + 64 + 32 positions");
static_assert((1 << (FOOTPRINT_LEVELS - 1)) <= 2 * FOOTPRINT_MAX_RADIUS + 1 && (1 << FOOTPRINT_LEVELS) > 2 * FOOTPRINT_MAX_RADIUS + 1, "the levels cover every width");
static_assert(FOOTPRINT_LINES % (4 * FOOTPRINT_BATCH) == 0, "whole batches per wavefront");

struct alignas(16) FootprintWord { // 128 positions of a line: bit i of lo is position x0 - 32 + i, bit i of hi position x0 + 32 + i
    unsigned long long lo, hi;
};

// the 64 bits of w from bit s on, 0 <= s <= 64
GG_DEV unsigned long long footprint_take(const FootprintWord &w, int s)
{
    return s >= 64 ? w.hi : (w.lo >> s) | ((w.hi << 1) << (63 - s));
}

GG_DEV uint32_t footprint_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_footprint_planes(const FootprintArgs x)
{
    __shared__ FootprintWord eroded[FOOTPRINT_LEVELS][FOOTPRINT_LINES];
    __shared__ uint2 fits[FOOTPRINT_MAX_HEADINGS][FOOTPRINT_TILE]; // (x: cells 0 .. 31 of the line, y: cells 32 .. 63)
    __shared__ uint32_t wave_counts[4][3];
    const uint32_t it = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int map = (int)(it / gridDim.x), tile = (int)(it % gridDim.x);
    const int nx = x.nx, ny = x.ny, R = x.radius, K = x.n_headings, D = 2 * R + 1;
    const int x0 = (tile % x.tiles_x) * FOOTPRINT_TILE, y0 = (tile / x.tiles_x) * FOOTPRINT_TILE;
    const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t *blocked = x.blocked + (size_t)map * x.blocked_stride;

    // ---- bitmap: the free cells of every line of the region, and their erosions
    {
        const int n_lines = FOOTPRINT_TILE + 2 * R, n_levels = x.n_levels;
        const int gx_lo = x0 - FOOTPRINT_MAX_RADIUS + lane, gx_hi = gx_lo + 64;
        const bool in_lo = gx_lo >= 0 && gx_lo < nx, in_hi = gx_hi < nx; // (gx_hi >= 32)
        // every lane loads, from an address clamped into the part of the line that is looked at (x0 - R .. x0 + 63 + R inside the map: never
        // empty, x0 < nx): a load under a condition is a branch and a wait of its own, and the loads of a batch would queue behind each other
        const int cx_lo = min(max(gx_lo, max(x0 - R, 0)), nx - 1), cx_hi = min(gx_hi, min(x0 + FOOTPRINT_TILE - 1 + R, nx - 1));
        const bool outside_blocked = x.outside_free == 0;
        for (int base = wave; base < n_lines; base += 4 * FOOTPRINT_BATCH) {
            int32_t v_lo[FOOTPRINT_BATCH], v_hi[FOOTPRINT_BATCH];
#pragma unroll
            for (int j = 0; j < FOOTPRINT_BATCH; ++j) {
                const int cy = min(max(y0 - R + base + 4 * j, 0), ny - 1); // (a line outside the map or beyond the region: loaded, not looked at)
                v_lo[j] = blocked[cy * nx + cx_lo];
                v_hi[j] = blocked[cy * nx + cx_hi];
            }
#pragma unroll
            for (int j = 0; j < FOOTPRINT_BATCH; ++j) {
                const int line = base + 4 * j, gy = y0 - R + line;
                const bool y_in = gy >= 0 && gy < ny;
                unsigned long long f_lo = ~__ballot(y_in && in_lo ? v_lo[j] >= 0 : outside_blocked); // (all 64 lanes are here)
                unsigned long long f_hi = ~__ballot(y_in && in_hi ? v_hi[j] >= 0 : outside_blocked);
                if (line >= n_lines) continue; // (uniform)
                for (int level = 0; level < FOOTPRINT_LEVELS; ++level) {
                    if (lane == level) eroded[level][line] = FootprintWord{f_lo, f_hi};
                    if (level + 1 >= n_levels) break; // (uniform; the shift below is at most 32)
                    const int p = 1 << level;
                    f_lo &= (f_lo >> p) | (f_hi << (64 - p));
                    f_hi &= f_hi >> p;
                }
            }
        }
    }
    __syncthreads();

    // ---- fits: per heading and line of the tile, the 64 cells of the line at which the heading fits
    for (int k = wave; k < K; k += 4) {
        const uint32_t *rows = x.table + k * D;
        unsigned long long all = ~0ull;
        for (int j = 0; j < D; ++j) {
            const uint32_t e = rows[j]; // (uniform)
            if (e == FOOTPRINT_EMPTY) continue;
            const FootprintWord w = eroded[e >> 16][lane + j]; // (line y0 + lane + a is line lane + a + R of the region)
            const int s1 = (int)(e & 0xFFu), s2 = (int)((e >> 8) & 0xFFu);
            all &= footprint_take(w, s1);
            if (s2 != s1) all &= footprint_take(w, s2); // (uniform: a width that is a power of two is one erosion word)
        }
        fits[k][lane] = make_uint2((uint32_t)all, (uint32_t)(all >> 32));
    }
    __syncthreads();

    // ---- gather: every cell its bits, the mask, the fit word, the counts
    uint32_t n_all = 0u, n_enough = 0u, n_none = 0u;
    const int gx = x0 + lane;
    for (int ly = wave; ly < FOOTPRINT_TILE; ly += 4) {
        const int gy = y0 + ly;
        if (gy >= ny) break; // (uniform)
        uint32_t m = 0u;
        for (int k = 0; k < K; ++k) m |= (((lane < 32 ? fits[k][ly].x : fits[k][ly].y) >> (lane & 31)) & 1u) << k; // (a broadcast per half)
        if (gx >= nx) continue; // (no cross-lane operation below)
        const int cell = gy * nx + gx, p = __popc(m);
        if (x.mask) x.mask[(size_t)map * x.mask_stride + (size_t)cell] = m;
        if (x.fit) x.fit[(size_t)map * x.fit_stride + (size_t)cell] = p >= x.min_fit ? -1 : p;
        n_all += p == K;
        n_enough += p >= x.min_fit;
        n_none += p == 0;
    }
    if (!x.counts) return; // (uniform)
    n_all = footprint_wave_sum(n_all); // (every lane is back here)
    n_enough = footprint_wave_sum(n_enough);
    n_none = footprint_wave_sum(n_none);
    if (lane == 0) {
        wave_counts[wave][0] = n_all;
        wave_counts[wave][1] = n_enough;
        wave_counts[wave][2] = n_none;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t *counts = x.counts + (size_t)map * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = (int)(wave_counts[0][c] + wave_counts[1][c] + wave_counts[2][c] + wave_counts[3][c]);
        if (v) atomicAdd(counts + c, v);
    }
}

void launch_footprint(const FootprintArgs &x, int n_maps, hipStream_t s)
{
    if (x.counts) (void)hipMemsetAsync(x.counts, 0, sizeof(int32_t) * 3 * (size_t)n_maps, s);
    const int tiles_y = (x.ny + FOOTPRINT_TILE - 1) / FOOTPRINT_TILE;
    hipLaunchKernelGGL(k_footprint_planes, dim3(x.tiles_x * tiles_y, n_maps), dim3(256), 0, s, x);
}

} // namespace gg
