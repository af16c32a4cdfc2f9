// region_args.h -- gg_cluster_planes (k26_regions.hip): what its launches share, and the launchers of k15_cluster.hip it drives.  A header
// of its own, included by gg_context.hip, k15_cluster.hip and k26_regions.hip alone: no other translation unit sees the call.
#pragma once

#include "gg_internal.h"

namespace gg {

// Map i of the call is row i of every buffer.  `forest` is a ClusterArgs on the d_cell_cluster planes WITHOUT per-cloud records
// (cl.clouds == nullptr: cluster_core.h cluster_io is the identity) and without a table (records == nullptr): k15_cluster.hip's merge,
// flatten, scan and rank launches run on it as they stand, and its n_clusters is call scratch
struct RegionArgs {
    ClusterArgs forest;
    const int32_t *seeds;          // map i's plane at seeds + i * seed_stride: a member where lo <= word <= hi
    size_t seed_stride;
    int lo, hi;
    int min_cells;                 // >= 1: a component of fewer cells is dropped
    const int32_t *values;         // map i's plane at values + i * value_stride; nullable
    size_t value_stride;
    uint32_t *sizes;               // the caller's d_cell_size as 32-bit words, map i's plane at sizes + i * size_stride; null: no size and no filter launch
    size_t size_stride;
    int32_t *heads;                // [map][4] K, dropped components, member cells, kept cells; nullable
    uint32_t *records;             // the caller's d_regions as 32-bit words, twelve per gg_region: [map][max_regions]; null: no table
    int max_regions;               // 0 without a table
    int tile;                      // 1: the tile-local stage (k_region_tile, k_region_rim) in place of the seed and the merge; the same results
};
constexpr int REGIONS_TILE_DEFAULT = 1; // (measured faster on every arm of tools/bench_regions.py: DESIGN.md K26)

void launch_cluster_forest(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s, bool merge); // k15_cluster.hip: (merge,) flatten on planes that hold L or 0xFFFFFFFF
void launch_cluster_ranks(const Arena &a, const ClusterArgs &x, int n_clouds, hipStream_t s);    // k15_cluster.hip: scan, rank behind the flatten (or a recount of the roots)
void launch_regions(const Arena &a, const RegionArgs &x, int n_maps, hipStream_t s);             // k26_regions.hip: tile, rim (or seed, merge), flatten, (sizes, filter,) scan, rank, init, apply, finalise

} // namespace gg
