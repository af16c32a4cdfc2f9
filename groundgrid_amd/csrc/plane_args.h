// The argument frame of the plane calls (gg_fuse_states, gg_track_clusters, gg_route_planes, gg_match_planes, gg_footprint_planes,
// gg_route_headings, gg_score_rollouts): the byte ranges of their device buffers and the test that no output shares a byte with another buffer, the clamp of
// a map's index shift, and the plane sides of an order.  Plain C++17: no HIP and no context (tests/cpp/test_plane_args.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <utility>

// [lo, hi): from a buffer's first word to the last word the call touches.  lo == nullptr: the buffer is not given
struct BufferRange {
    const char *name, *lo, *hi;
    bool out;
};

// n planes (volumes) of `words` 4-byte words, `stride` words apart: the range ends with the last plane, not with the last stride
inline BufferRange plane_range(const char *name, const void *p, int n, size_t stride, size_t words, bool out)
{
    return {name, (const char *)p, p ? (const char *)p + ((size_t)(n - 1) * stride + words) * 4 : nullptr, out};
}
// n rows of `bytes` bytes, one behind the other
inline BufferRange row_range(const char *name, const void *p, int n, size_t bytes, bool out)
{
    return {name, (const char *)p, p ? (const char *)p + (size_t)n * bytes : nullptr, out};
}

// The first pair of given ranges that share a byte and of which at least one is an output, in table order (the earlier range first,
// every later range against it before the next); {-1, -1} when there is none.  Ranges that touch do not overlap; two inputs may.
// (A table of one input and outputs only tests every pair: each pair holds an output.  That is gg_footprint_planes' rule.)
inline std::pair<int, int> first_overlap(const BufferRange *ranges, int count)
{
    const std::less<const char *> before;
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j) {
            const BufferRange &p = ranges[i], &q = ranges[j];
            if (!p.lo || !q.lo || !(p.out || q.out)) continue;
            if (before(p.lo, q.hi) && before(q.lo, p.hi)) return {i, j};
        }
    return {-1, -1};
}

struct Shift {
    int s0, s1;
};
// shifts[2 i], shifts[2 i + 1] in (rows, cols), clamped to [-rows, rows] x [-cols, cols]: from |s| = side on nothing lies inside the map.
// (rows, cols) as given: the caller lays them along and across the lines of its order
inline Shift clamped_shift(const int32_t *shifts, int i, int rows, int cols)
{
    return {std::min(std::max(shifts[2 * (size_t)i], -rows), rows), std::min(std::max(shifts[2 * (size_t)i + 1], -cols), cols)};
}

// (cells along a line of the plane, lines) of a map of rows x cols in either order
inline std::pair<int, int> plane_sides(bool row_major, int rows, int cols) { return row_major ? std::make_pair(cols, rows) : std::make_pair(rows, cols); }
