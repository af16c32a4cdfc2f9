// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// pcl/point_types.h: the macros velodyne_pointcloud/point_types.h uses, so that its PointXYZIR is the 32-byte, 16-byte aligned record
// of gg_point32 (x, y, z, one float of padding, intensity, ring); the point-struct registration expands to nothing.
#pragma once

#include <cstdint>

#define EIGEN_ALIGN16 __attribute__((aligned(16)))
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#define PCL_ADD_POINT4D              \
    union EIGEN_ALIGN16 {            \
        float data[4];               \
        struct {                     \
            float x;                 \
            float y;                 \
            float z;                 \
        };                           \
    }
#define POINT_CLOUD_REGISTER_POINT_STRUCT(name, seq)
