// cluster_core.h -- the lock-free forest of the connected-components calls: what k15_cluster.hip (gg_cluster_clouds) and k26_regions.hip
// (gg_cluster_planes) share on the device.  A plane of one 32-bit word per cell is the forest: CLUSTER_EMPTY on a cell that takes no part,
// else a parent pointer.  Its ONLY write is atomicMin(parent[larger root], smaller root): a parent only ever decreases, so every chain is
// strictly descending (find takes at most rows * cols steps and a union, whose larger end strictly decreases from try to try, at most
// 2 * rows * cols tries), and the root of a finished component is its smallest cell index -- whatever the order of the unions.  A stale
// parent (these loads ask for no freshness beyond a launch boundary) is a former ancestor of the same component: it costs steps or a retry,
// because the atomic's return value is the truth, never a wrong union.
#pragma once

#include "cloud_walk.h"

namespace gg {

constexpr uint32_t CLUSTER_EMPTY = 0xFFFFFFFFu; // an unoccupied cell, from the seed on (-1 as the caller reads it)
constexpr int CLUSTER_WAVE_ROUNDS = 4; // ids a wavefront reduces over its lanes before the remaining lanes send their own atomics

GG_DEV uint32_t cluster_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (map, 256-cell chunk) of a work-group of the cell launches, grid (cell_chunks, clouds)
GG_DEV void cluster_cell_item(int &cloud, int &chunk)
{
    const uint32_t item = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    cloud = (int)(item / gridDim.x);
    chunk = (int)(item % gridDim.x);
}

// the row of the caller's buffers of the call's map `cloud`: its record's io_index, or -- a plane call, which has no records -- the map itself
GG_DEV int cluster_io(const ClusterArgs &x, int cloud) { return x.cl.clouds ? x.cl.clouds[cloud].io_index : cloud; }

// The lanes of a large cluster's interior all hold one id: one lane speaks for a run of them.  At most CLUSTER_WAVE_ROUNDS times, the first
// lane that still holds an id (rid >= 0) names it and run(id, mine, count, speaker) is called by ALL lanes (it reduces over the lanes with
// `mine`, and the `speaker` lane sends the result for the `count` of them); those lanes' rid becomes -1.  A lane whose rid is still >= 0
// afterwards sends its own.  To be called in wavefront-uniform control flow.
template <class Run> GG_DEV void cluster_id_runs(int &rid, int lane, Run &&run)
{
    unsigned long long todo = __ballot(rid >= 0);
    for (int round = 0; round < CLUSTER_WAVE_ROUNDS && todo; ++round) {
        const int src = __ffsll((long long)todo) - 1;
        const int cur = __shfl(rid, src, 64);
        const bool mine = rid == cur;
        const unsigned long long m = __ballot(mine);
        run(cur, mine, (int)__popcll(m), lane == src);
        if (mine) rid = -1;
        todo &= ~m;
    }
}

// find: at most x steps (every step goes to a smaller index; a word that is no smaller index ends the walk)
GG_DEV uint32_t cluster_find(const uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = cluster_load(parent + x);
        if (p >= x) return x;
        x = p;
    }
}
// union: a + b strictly decreases from try to try
GG_DEV void cluster_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cluster_find(parent, a);
        b = cluster_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return; // a was a root and hangs under b now
        a = old;              // a had the parent `old` (< a): parent[a] is min(old, b) now, and what is left to unite is old with b
    }
}

} // namespace gg
