// plane_args.h alone (no HIP, no context): the ranges of the plane calls' buffers, the overlap test and the shift clamp.
#include "plane_args.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static bool same(std::pair<int, int> got, int i, int j) { return got.first == i && got.second == j; }

int main()
{
    static int32_t buf[4096];
    const char *base = (const char *)buf;
    // the end of a range: the last plane, not the last stride; one plane; rows
    BufferRange r = plane_range("a", buf, 3, 416, 400, true);
    CHECK(r.lo == base && r.hi == base + (2 * 416 + 400) * 4 && r.out);
    r = plane_range("a", buf, 1, 1000000, 400, false);
    CHECK(r.hi == base + 400 * 4 && !r.out);
    r = plane_range("a", buf + 7, 2, 50, 18, true); // (a volume smaller than a plane)
    CHECK(r.lo == base + 28 && r.hi == base + 28 + (50 + 18) * 4);
    r = row_range("a", buf, 3, 32, true);
    CHECK(r.hi == base + 96);
    r = plane_range("a", nullptr, 3, 416, 400, true);
    CHECK(!r.lo && !r.hi);
    r = row_range("a", nullptr, 3, 32, true);
    CHECK(!r.lo && !r.hi);

    // touching ranges do not overlap, on either side
    BufferRange t[4] = {plane_range("in", buf, 2, 100, 100, false), plane_range("out", buf + 200, 2, 100, 100, true)};
    CHECK(same(first_overlap(t, 2), -1, -1));
    t[1] = plane_range("out", buf, 2, 100, 100, true);
    t[0] = plane_range("in", buf + 200, 2, 100, 100, false);
    CHECK(same(first_overlap(t, 2), -1, -1));
    // apart
    t[0] = plane_range("in", buf + 1000, 2, 100, 100, false);
    CHECK(same(first_overlap(t, 2), -1, -1));
    // the last word of the last plane, and the first word
    t[0] = plane_range("in", buf, 2, 116, 100, false); // ends behind word 215
    t[1] = plane_range("out", buf + 215, 1, 100, 100, true);
    CHECK(same(first_overlap(t, 2), 0, 1));
    t[1] = plane_range("out", buf + 216, 1, 100, 100, true);
    CHECK(same(first_overlap(t, 2), -1, -1));
    t[1] = plane_range("out", buf, 1, 100, 1, true);
    CHECK(same(first_overlap(t, 2), 0, 1));
    // the slack between two planes belongs to the range: what lies there overlaps
    t[1] = plane_range("out", buf + 104, 1, 8, 8, true);
    CHECK(same(first_overlap(t, 2), 0, 1));
    // a buffer that is not given is skipped, whatever its other members say
    t[1] = BufferRange{"out", nullptr, base + 4096, true};
    CHECK(same(first_overlap(t, 2), -1, -1));
    // two inputs may share everything; an output with either may not
    t[0] = plane_range("in0", buf, 2, 100, 100, false);
    t[1] = plane_range("in1", buf, 2, 100, 100, false);
    CHECK(same(first_overlap(t, 2), -1, -1));
    t[2] = plane_range("out", buf + 199, 1, 4, 4, true);
    CHECK(same(first_overlap(t, 3), 0, 2));
    // several pairs overlap: the earliest first range wins, then its earliest partner
    t[0] = plane_range("in0", buf + 2000, 1, 10, 10, false);
    t[1] = plane_range("in1", buf, 1, 10, 10, false);
    t[2] = plane_range("out0", buf + 5, 1, 10, 10, true);    // on in1 and on out1
    t[3] = plane_range("out1", buf + 2005, 1, 10, 10, true); // on in0
    CHECK(same(first_overlap(t, 4), 0, 3));
    t[3] = plane_range("out1", buf + 8, 1, 10, 10, true); // on in1 and on out0
    CHECK(same(first_overlap(t, 4), 1, 2));
    t[2] = plane_range("out0", buf + 3000, 1, 10, 10, true);
    CHECK(same(first_overlap(t, 4), 1, 3));
    CHECK(same(first_overlap(t, 0), -1, -1));

    // the clamp: inside, at the side, beyond it, at the ends of int32
    const int32_t s[10] = {3, -4, 20, -30, -20, 30, 21, -31, INT32_MAX, INT32_MIN};
    Shift c = clamped_shift(s, 0, 20, 30);
    CHECK(c.s0 == 3 && c.s1 == -4);
    c = clamped_shift(s, 1, 20, 30);
    CHECK(c.s0 == 20 && c.s1 == -30);
    c = clamped_shift(s, 2, 20, 30);
    CHECK(c.s0 == -20 && c.s1 == 30);
    c = clamped_shift(s, 3, 20, 30);
    CHECK(c.s0 == 20 && c.s1 == -30);
    c = clamped_shift(s, 4, 20, 30);
    CHECK(c.s0 == 20 && c.s1 == -30);

    CHECK(plane_sides(true, 20, 30) == std::make_pair(30, 20) && plane_sides(false, 20, 30) == std::make_pair(20, 30));
    std::printf("plane args OK\n");
    return 0;
}
