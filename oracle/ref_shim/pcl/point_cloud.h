// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// pcl/point_cloud.h: pcl::PointCloud<T> with ::Ptr and points (a std::vector: with C++17 its emplace_back returns a reference and
// its allocator honours the points' alignment).
#pragma once

#include <pcl/point_types.h>

#include <memory>
#include <vector>

namespace pcl {
template <typename PointT> class PointCloud {
public:
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
    std::vector<PointT> points;
    std::size_t size() const { return points.size(); }
};
} // namespace pcl
